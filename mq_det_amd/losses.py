"""The ATSS training objective of MQ-GLIP, evaluated forward-only on the device (csrc/atss_loss.hip).

Reference: maskrcnn_benchmark/modeling/rpn/loss.py ATSSLossComputation.prepare_targets (:655-832) and __call__ (:850-1201) under the loss
switches of configs/pretrain/mq-glip-*.yaml (USE_DOT_PRODUCT_TOKEN_LOSS; classification / token / contrastive / shallow / MLM losses off; one
anchor per location).  This is NOT a training mode: there is no autograd and `model.train()` keeps raising.  What it serves: choosing between
checkpoints by held-out loss (`evaluate_loss`), and handing the reference's own trainer its targets (`prepare_targets`).

  prepare_targets(targets, anchors, positive_map, topk)      -> the reference's (cls_labels, reg_targets, token_labels), on the device
  ATSSLoss(cfg)(head, anchors, targets, positive_map, masks) -> the reference's loss dict + the raw sums and counts
  evaluate_loss(model, data_loader)                          -> dataset means of the three losses, one host synchronisation

Deliberate difference: an image without gt boxes is all background here; the reference's `ious_inf.max(dim=1)` fails on the empty dimension.
"""
import torch

from . import ops

# (config key path, the value this path implements)
_SWITCHES = (("USE_DOT_PRODUCT_TOKEN_LOSS", True), ("USE_CLASSIFICATION_LOSS", False), ("USE_TOKEN_LOSS", False),
             ("USE_CONTRASTIVE_ALIGN_LOSS", False), ("USE_SHALLOW_CONTRASTIVE_LOSS", False), ("USE_BACKBONE_SHALLOW_CONTRASTIVE_LOSS", False),
             ("MLM_LOSS", False))
_SWITCH_DEFAULT = {"USE_DOT_PRODUCT_TOKEN_LOSS": True}
SUM_NAMES = ("num_pos", "sum_centerness", "sum_giou_weighted", "sum_centerness_bce", "sum_giou", "sum_token")


def validate_loss_config(cfg):
    """Raise NotImplementedError, naming the key, for every loss setting of the reference this path does not evaluate."""
    fc = cfg.MODEL.DYHEAD.FUSE_CONFIG
    for key, want in _SWITCHES:
        got = bool(fc.get(key, _SWITCH_DEFAULT.get(key, False)))
        if got != want:
            raise NotImplementedError(f"MODEL.DYHEAD.FUSE_CONFIG.{key} = {got}: the device loss evaluates the mq-glip-*.yaml objective only "
                                      f"({key} {want})")
    rpn = cfg.MODEL.RPN
    if len(tuple(rpn.ASPECT_RATIOS)) != 1:
        raise NotImplementedError(f"MODEL.RPN.ASPECT_RATIOS = {tuple(rpn.ASPECT_RATIOS)}: one anchor per location")
    if int(rpn.SCALES_PER_OCTAVE) != 1:
        raise NotImplementedError(f"MODEL.RPN.SCALES_PER_OCTAVE = {rpn.SCALES_PER_OCTAVE}: one anchor per location")
    topk = int(cfg.MODEL.ATSS.get("TOPK", 9))
    if not 1 <= topk <= ops.ATSS_MAX_TOPK:
        raise NotImplementedError(f"MODEL.ATSS.TOPK = {topk}: 1 .. {ops.ATSS_MAX_TOPK}")


def _anchor_tensor(anchors):
    """-> ([A, 4] fp32 contiguous, [anchors per level]).  Accepts the project's per-level tensors, or the reference's list (per image) of
    lists (per level) of BoxLists -- every image of a batch shares one padded canvas, so the first image's anchors serve all."""
    if len(anchors) and isinstance(anchors[0], (list, tuple)):
        anchors = anchors[0]
    levels = [a.bbox if hasattr(a, "bbox") else a for a in anchors]
    if not levels or any(not torch.is_tensor(a) or a.dim() != 2 or a.shape[1] != 4 for a in levels):
        raise ValueError("anchors: one [n, 4] tensor (or BoxList) per pyramid level")
    return torch.cat([a.float() for a in levels]).contiguous(), [a.shape[0] for a in levels]


def _upload(t, device):
    """`t` on `device` without the host waiting for the device: host memory goes through a pinned staging copy (the caching host allocator
    keeps it until the copy has run), as ops.eval_rows_table does."""
    device = torch.device(device)
    if t.device == device:
        return t
    if t.device.type == "cpu" and device.type == "cuda":
        t = t.pin_memory()
    return t.to(device, non_blocking=True)


def _pack_targets(targets, device):
    """list[BoxList] -> (gt [G, 4] fp32, labels [G] int64, gt_off [B + 1] int32 on the device, host counts).  No device->host transfer."""
    if not isinstance(targets, (list, tuple)) or len(targets) == 0:
        raise ValueError("targets: a non-empty list of BoxLists, one per image")
    for t in targets:
        if not (hasattr(t, "bbox") and hasattr(t, "mode") and hasattr(t, "get_field")):
            raise ValueError(f"targets: BoxLists expected, got {type(t).__name__}")
        if t.mode != "xyxy":
            raise ValueError(f"targets: BoxLists in 'xyxy' mode expected, got '{t.mode}'")
        if "labels" not in t.fields():
            raise ValueError("targets: every BoxList needs a 'labels' field")
        if len(t.get_field("labels")) != len(t.bbox):
            raise ValueError("targets: 'labels' and boxes differ in length")
    counts = [int(t.bbox.shape[0]) for t in targets]
    # (uploads from host memory are asynchronous: the host never waits for the device here)
    gt = _upload(torch.cat([t.bbox.reshape(-1, 4).float() for t in targets]).contiguous(), device)
    labels = _upload(torch.cat([t.get_field("labels").reshape(-1).long() for t in targets]).contiguous(), device)
    offs = [0]
    for c in counts:
        offs.append(offs[-1] + c)
    return gt, labels, _upload(torch.tensor(offs, dtype=torch.int32), device), counts


def _positive_map_tensor(positive_map, total, device):
    if not torch.is_tensor(positive_map) or positive_map.dim() != 2 or positive_map.shape[0] != total:
        raise ValueError(f"positive_map: a [{total}, T] tensor expected (one row per gt box of the batch, image after image)")
    return _upload(positive_map.float().contiguous(), device)


def assign(targets, anchors, topk=9):
    """-> (matched [B, A] int32: the gt's index inside its image or -1, and the packed tensors the other kernels take)."""
    flat, sizes = _anchor_tensor(anchors)
    gt, labels, gt_off, counts = _pack_targets(targets, flat.device)
    matched = ops.atss_assign(flat, sizes, gt, gt_off, len(targets), topk)
    return matched, {"anchors": flat, "sizes": sizes, "gt": gt, "labels": labels, "gt_off": gt_off, "counts": counts}


@torch.no_grad()
def prepare_targets(targets, anchors, positive_map=None, topk=9):
    """ATSSLossComputation.prepare_targets (rpn/loss.py:655-832) for a batch, on the device: -> (cls_labels, reg_targets, token_labels), lists
    per image of [A] int64, [A, 4] fp32 and [A, T] fp32 (token_labels is empty without `positive_map`), what a reference trainer splices in.
    targets: BoxLists in xyxy mode with a 'labels' field, in input-image coordinates (anything else: ValueError); anchors: per-level [n, 4]
    tensors (or the reference's per-image lists of BoxLists); positive_map [sum of gts, T].  An image without gts is all background."""
    matched, pk = assign(targets, anchors, topk)
    _, cls, reg = ops.atss_box_loss(pk["anchors"], pk["gt"], pk["labels"], pk["gt_off"], matched, want_targets=True)
    B = len(targets)
    token_labels = []
    if positive_map is not None:
        pm = _positive_map_tensor(positive_map, len(pk["gt"]), matched.device)
        unmatched = torch.zeros(pm.shape[1], dtype=pm.dtype, device=pm.device)
        unmatched[-1] = 1
        off = 0
        for b in range(B):
            m = matched[b].long()
            if pk["counts"][b]:
                rows = pm[off:off + pk["counts"][b]][m.clamp(min=0)]
                rows[m < 0] = unmatched
            else:
                rows = unmatched.expand(m.shape[0], -1).clone()
            token_labels.append(rows)
            off += pk["counts"][b]
    return [cls[b] for b in range(B)], [reg[b] for b in range(B)], token_labels


def _token_loss_plain(logits, matched, pm, gt_off_host, text_mask, alpha, gamma):
    """The plain path (GEMM fallback head): token_sigmoid_binary_focal_loss on materialised logits [B, A, T], summed."""
    import torch.nn.functional as F
    B, A, T = logits.shape
    total = logits.new_zeros(())
    for b in range(B):
        m = matched[b].long()
        tgt = logits.new_zeros(A, pm.shape[1])
        if gt_off_host[b + 1] > gt_off_host[b]:
            tgt = pm[gt_off_host[b]:gt_off_host[b + 1]][m.clamp(min=0)].clone()
        bg = m < 0
        tgt[bg] = 0
        tgt[bg, -1] = 1
        tgt = tgt[:, :T]
        x = logits[b].float()
        p = torch.sigmoid(x)
        ce = F.binary_cross_entropy_with_logits(x, tgt, reduction="none")
        loss = ce * (1 - (p * tgt + (1 - p) * (1 - tgt))) ** gamma
        if alpha >= 0:
            loss = (alpha * tgt + (1 - alpha) * (1 - tgt)) * loss
        total = total + (loss * (text_mask[b, :T] > 0)).sum()
    return total.reshape(1)


def _world():
    import torch.distributed as dist
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


class ATSSLoss:
    """ATSSLossComputation.__call__ for the MQ-GLIP objective.  `head` is what the head stage hands to `postprocess`: the fused form
    (`tok`, `tk16`, `tbias`, `wbc`, `bbc`, `scales`, `sizes`, `max_kv`: the token loss is formed by mq_token_focal_loss_fwd without writing
    logits) or the GEMM-fallback form (`bbox_reg`, `centerness`, `dot`, `tbias`: captions over 256 tokens etc.; the logits exist already and a
    plain torch path evaluates the loss on them).  A head may also carry `reg` [B, A, 4] / `ctr` [B, A] fp32 directly."""

    def __init__(self, cfg):
        validate_loss_config(cfg)
        self.cfg = cfg
        fc = cfg.MODEL.DYHEAD.FUSE_CONFIG
        self.topk = int(cfg.MODEL.ATSS.get("TOPK", 9))
        self.reg_weight = float(cfg.MODEL.ATSS.get("REG_LOSS_WEIGHT", 2.0))
        self.alpha, self.gamma = float(fc.get("TOKEN_ALPHA", 0.25)), float(fc.get("TOKEN_GAMMA", 2.0))
        self.token_weight = float(fc.get("DOT_PRODUCT_TOKEN_LOSS_WEIGHT", 1.0))

    @staticmethod
    def _box_outputs(head):
        """reg [B, A, 4] and ctr [B, A] fp32 of a head dict."""
        if "reg" in head and "ctr" in head:
            return head["reg"].float().contiguous(), head["ctr"].float().contiguous()
        if "tok" in head:
            # the box / centerness rows come out of the alignment kernel (their only producer): one label, one token, scores unused
            tokidx = torch.zeros(1, 1, dtype=torch.int32, device=head["tok"].device)
            fused = ops.align_fused(head["tok"], head["tk16"], head["tbias"], head["wbc"], head["bbc"], head["scales"], tokidx, head["sizes"],
                                    2.0, kv_max=head.get("max_kv", 0))
            return torch.cat(fused["reg"], 1).contiguous(), fused["ctr"]
        B = head["tbias"].shape[0]
        reg = torch.cat([r.permute(0, 2, 3, 1).reshape(B, -1, 4) for r in head["bbox_reg"]], 1).float().contiguous()
        ctr = torch.cat([c.permute(0, 2, 3, 1).reshape(B, -1) for c in head["centerness"]], 1).float().contiguous()
        return reg, ctr

    @torch.no_grad()
    def __call__(self, head, anchors, targets, positive_map, text_masks):
        validate_loss_config(self.cfg)                            # before the first launch, and again if the cfg was edited since
        matched, pk = assign(targets, anchors, self.topk)
        dev = matched.device
        B, A = matched.shape
        pm = _positive_map_tensor(positive_map, len(pk["gt"]), dev)
        T = head["tbias"].shape[1]
        if pm.shape[1] < T or text_masks.shape[0] != B or text_masks.shape[1] < T:
            raise ValueError(f"positive_map [{tuple(pm.shape)}] / text_masks [{tuple(text_masks.shape)}] are narrower than the head's {T} text positions")
        mask = text_masks[:, :T].to(device=dev, dtype=torch.int32).contiguous()
        reg, ctr = self._box_outputs(head)
        if reg.shape != (B, A, 4) or ctr.shape != (B, A):
            raise ValueError(f"head: box outputs {tuple(reg.shape)} / {tuple(ctr.shape)} for {B} images of {A} anchors")
        sums, _, _ = ops.atss_box_loss(pk["anchors"], pk["gt"], pk["labels"], pk["gt_off"], matched, reg, ctr)
        if "tok" in head and head["tok"].shape[1] == A:
            tok_sum = ops.token_focal_loss(head["tok"], head["tk16"], head["tbias"], matched, pm, pk["gt_off"], mask, self.alpha, self.gamma,
                                           kv_max=head.get("max_kv", 0))
        else:
            dot = head["logits"] if "logits" in head else torch.cat(list(head["dot"]), 1)
            logits = (dot.float() + head["tbias"][:, None, :]).clamp(-50000, 50000)
            offs = [0]
            for c in pk["counts"]:
                offs.append(offs[-1] + c)
            tok_sum = _token_loss_plain(logits, matched, pm, offs, mask, self.alpha, self.gamma)
        raw = torch.cat([sums, tok_sum])                          # SUM_NAMES, on the device
        out = self.losses_from_sums(raw)
        out["sums"] = raw
        out["matched"] = matched
        return out

    def losses_from_sums(self, raw):
        """The reference's normalisation of one batch's sums (rpn/loss.py:1147-1201), on the device: max(num_pos / world, 1) and
        sum centerness / world with num_pos and the centerness sum all-reduced when torch.distributed is initialised."""
        world = _world()
        red = raw[:2].clone()
        if world > 1:
            import torch.distributed as dist
            dist.all_reduce(red)
        npos_avg = (red[0] / world).clamp(min=1.0)
        ct_avg = red[1] / world
        zero = raw.new_zeros(())
        has_pos = raw[0] > 0
        # GIoULoss: weighted by the centerness targets when their (local) sum is positive, else the plain sum; no positives: empty sums
        giou = torch.where(raw[1] > 0, raw[2], raw[4])
        return {"loss_reg": torch.where(has_pos, giou / ct_avg, zero) * self.reg_weight,
                "loss_centerness": torch.where(has_pos, raw[3] / npos_avg, zero),
                "loss_dot_product_token": raw[5] / npos_avg * self.token_weight,
                "loss_cls": zero.clone()}


@torch.no_grad()
def evaluate_loss(model, data_loader, device="cuda"):
    """Dataset means of the three losses from the raw sums: sum over batches first, normalise once -- loss_reg = REG_LOSS_WEIGHT S ct (1 - GIoU)
    / S ct, loss_centerness = S BCE / max(positives, 1), loss_dot_product_token = WEIGHT S focal / max(positives, 1).  A batch is
    (images, targets, ...) as the reference's loaders yield it; captions come from the targets' 'caption' field, the positive map from their
    'positive_map' field.  ONE host synchronisation, at the end.  -> dict of floats (+ 'num_pos', 'batches').
    An MQ-GroundingDINO model (cfg.GROUNDINGDINO.enabled) is evaluated on its set criterion instead: set_loss.evaluate_set_loss."""
    if model.cfg.get("GROUNDINGDINO", {}).get("enabled", False):
        from .set_loss import evaluate_set_loss
        return evaluate_set_loss(model, data_loader, device)
    model.eval()
    crit = ATSSLoss(model.cfg)
    total, n = None, 0
    for batch in data_loader:
        images, targets = batch[0], batch[1]
        captions = [t.get_field("caption") for t in targets]
        out = model.forward_losses(images.to(device) if hasattr(images, "to") else images, targets, captions)
        total = out["sums"].double() if total is None else total + out["sums"].double()
        n += 1
    if total is None:
        raise ValueError("evaluate_loss: the data loader yielded no batch")
    if _world() > 1:
        import torch.distributed as dist
        dist.all_reduce(total)
    s = dict(zip(SUM_NAMES, total.tolist()))                     # the one device->host transfer
    npos = max(s["num_pos"], 1.0)
    giou = s["sum_giou_weighted"] if s["sum_centerness"] > 0 else s["sum_giou"]
    return {"loss_reg": crit.reg_weight * giou / (s["sum_centerness"] or float("nan")) if s["num_pos"] > 0 else 0.0,
            "loss_centerness": s["sum_centerness_bce"] / npos if s["num_pos"] > 0 else 0.0,
            "loss_dot_product_token": crit.token_weight * s["sum_token"] / npos,
            "num_pos": int(s["num_pos"]), "batches": n}
