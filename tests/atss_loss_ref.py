"""TEST INFRASTRUCTURE: a from-scratch torch restatement of ATSS target assignment and the MQ-GLIP loss terms (written for the tests of
mq_det_amd/losses.py from the algorithm's description -- per-level nearest-k, mean + std threshold, centre test, best IoU; BoxCoder targets;
centerness; GIoU; token focal loss -- not from the reference's text), the integer-draw recipes of the fixture head outputs, and the fp64
margins of the four conditions under which assignment is a function of its inputs at all (tests/golden/atss_loss, tools/gen_golden_atss_loss.py).

The restatement is a per-image loop over dense [A, G] matrices with materialised [A, T] logits: also the baseline tools/atss_loss_bench.py times."""
import hashlib
import math

import numpy as np
import torch

STRIDES = (8, 16, 32, 64, 128)
ANCHOR_SIZES = (64, 128, 256, 512, 1024)
MARGINS = {"kth_gap": 1e-3, "thr": 1e-5, "centre": 1e-3, "tie": 1e-6}       # the conditions of the issue, in its order
CLIP = math.log(1000.0 / 16)


def level_sizes(h, w, strides=STRIDES):
    return [(-(-h // s), -(-w // s)) for s in strides]


def cell_anchors(strides=STRIDES, sizes=ANCHOR_SIZES):
    """one square anchor per location, centred on (stride - 1) / 2 with the legacy inclusive width: [c - (size - 1) / 2, c + (size - 1) / 2]"""
    out = []
    for s, a in zip(strides, sizes):
        c, h = (s - 1) / 2.0, (a - 1) / 2.0
        out.append([c - h, c - h, c + h, c + h])
    return torch.tensor(out, dtype=torch.float32)


def grid_anchors(sizes, cells, strides=STRIDES, device="cpu"):
    out = []
    for (H, W), s, cell in zip(sizes, strides, cells):
        xs = torch.arange(W, dtype=torch.float32, device=device) * s
        ys = torch.arange(H, dtype=torch.float32, device=device) * s
        yy, xx = torch.meshgrid(ys, xs, indexing="ij")
        sh = torch.stack([xx.reshape(-1), yy.reshape(-1), xx.reshape(-1), yy.reshape(-1)], 1)
        out.append((sh + cell.to(device)[None]).contiguous())
    return out


# ------------------------------------------------------------------------------------------------ assignment
def _iou(a, g):
    """[A, 4] x [G, 4] -> [A, G], inclusive pixel convention"""
    area_a = (a[:, 2] - a[:, 0] + 1) * (a[:, 3] - a[:, 1] + 1)
    area_g = (g[:, 2] - g[:, 0] + 1) * (g[:, 3] - g[:, 1] + 1)
    w = (torch.minimum(a[:, None, 2], g[None, :, 2]) - torch.maximum(a[:, None, 0], g[None, :, 0]) + 1).clamp(min=0)
    h = (torch.minimum(a[:, None, 3], g[None, :, 3]) - torch.maximum(a[:, None, 1], g[None, :, 1]) + 1).clamp(min=0)
    inter = w * h
    return inter / (area_a[:, None] + area_g[None] - inter)


def assign_image(levels, gt, topk=9, dtype=torch.float32, want_margins=False):
    """One image: levels = per-level [n, 4] anchors, gt [G, 4] -> matched [A] int64 (-1 background) [, margins dict in `dtype`]."""
    anchors = torch.cat(levels).to(dtype)
    gt = gt.to(dtype)
    A, G = anchors.shape[0], gt.shape[0]
    if G == 0:
        m = torch.full((A,), -1, dtype=torch.int64, device=anchors.device)
        return (m, {k: float("inf") for k in MARGINS}) if want_margins else m
    iou = _iou(anchors, gt)
    ac = torch.stack([(anchors[:, 0] + anchors[:, 2]) / 2, (anchors[:, 1] + anchors[:, 3]) / 2], 1)
    gc = torch.stack([(gt[:, 0] + gt[:, 2]) / 2, (gt[:, 1] + gt[:, 3]) / 2], 1)
    dist = (ac[:, None, :] - gc[None]).pow(2).sum(-1).sqrt()                    # [A, G]
    cand = torch.zeros(A, G, dtype=torch.bool, device=anchors.device)
    gap = float("inf")
    lo = 0
    for lv in levels:
        n = lv.shape[0]
        k = min(topk, n)
        d, order = torch.sort(dist[lo:lo + n], dim=0, stable=True)               # a tie: the lower anchor index first
        cand[lo:lo + n].scatter_(0, order[:k], True)
        if n > k:
            gap = min(gap, float((d[k] - d[k - 1]).min()))
        lo += n
    ncand = cand.sum(0)
    ci = torch.where(cand, iou, torch.zeros_like(iou))
    mean = ci.sum(0) / ncand
    var = (torch.where(cand, (iou - mean[None]) ** 2, torch.zeros_like(iou))).sum(0) / (ncand - 1)
    thr = mean + var.sqrt()
    inside = torch.stack([ac[:, None, 0] - gt[None, :, 0], ac[:, None, 1] - gt[None, :, 1],
                          gt[None, :, 2] - ac[:, None, 0], gt[None, :, 3] - ac[:, None, 1]], -1).min(-1).values
    pos = cand & (iou >= thr[None]) & (inside > 0.01)
    score = torch.where(pos, iou, torch.full_like(iou, -1.0))
    best, arg = score.max(1)                                                     # (first maximum = the lower gt on CPU; ties are excluded by condition 4)
    matched = torch.where(best >= 0, arg, torch.full_like(arg, -1))
    if not want_margins:
        return matched
    two = torch.topk(score, min(2, G), dim=1).values
    claimed_twice = pos.sum(1) > 1
    tie = float((two[claimed_twice, 0] - two[claimed_twice, 1]).min()) if G > 1 and bool(claimed_twice.any()) else float("inf")
    margins = {"kth_gap": gap, "thr": float((iou - thr[None]).abs()[cand].min()), "centre": float((inside - 0.01).abs()[cand].min()), "tie": tie}
    return matched, margins


def conditions_hold(levels, gts, topk=9):
    """The four conditions in fp64 over a batch -> (ok, {name: worst margin})."""
    worst = {k: float("inf") for k in MARGINS}
    for gt in gts:
        _, m = assign_image([l.double() for l in levels], gt.double(), topk, torch.float64, want_margins=True)
        for k in worst:
            worst[k] = min(worst[k], m[k])
    return all(worst[k] >= MARGINS[k] for k in MARGINS), worst


# ------------------------------------------------------------------------------------------------ targets and losses
def encode(gt, anchors):
    aw, ah = anchors[:, 2] - anchors[:, 0] + 1, anchors[:, 3] - anchors[:, 1] + 1
    ax, ay = anchors[:, 0] + 0.5 * aw, anchors[:, 1] + 0.5 * ah
    gw, gh = gt[:, 2] - gt[:, 0] + 1, gt[:, 3] - gt[:, 1] + 1
    gx, gy = gt[:, 0] + 0.5 * gw, gt[:, 1] + 0.5 * gh
    return torch.stack([10 * (gx - ax) / aw, 10 * (gy - ay) / ah, 5 * torch.log(gw / aw), 5 * torch.log(gh / ah)], 1)


def decode(code, anchors):
    aw, ah = anchors[:, 2] - anchors[:, 0] + 1, anchors[:, 3] - anchors[:, 1] + 1
    ax, ay = anchors[:, 0] + 0.5 * aw, anchors[:, 1] + 0.5 * ah
    cx, cy = code[:, 0] / 10 * aw + ax, code[:, 1] / 10 * ah + ay
    w, h = torch.exp((code[:, 2] / 5).clamp(max=CLIP)) * aw, torch.exp((code[:, 3] / 5).clamp(max=CLIP)) * ah
    return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w - 1, cy + 0.5 * h - 1], 1)


def targets_image(levels, gt, labels, matched):
    """-> (cls [A] int64, reg [A, 4]); a background anchor carries the encoding of gt 0 (zeros in an image without gts)"""
    anchors = torch.cat(levels)
    if gt.shape[0] == 0:
        return torch.zeros(len(anchors), dtype=torch.int64, device=anchors.device), torch.zeros_like(anchors)
    idx = matched.clamp(min=0)
    cls = torch.where(matched >= 0, labels[idx], torch.zeros_like(labels[idx]))
    return cls, encode(gt[idx].to(anchors.dtype), anchors)


def box_sums_image(levels, gt, labels, matched, reg, ctr):
    """-> [5]: positives, S ct, S ct (1 - GIoU), S BCE(ctr, ct), S (1 - GIoU), in reg's dtype"""
    anchors = torch.cat(levels).to(reg.dtype)
    cls, tgt = targets_image([anchors], gt.to(reg.dtype), labels, matched)
    pos = cls > 0
    if not bool(pos.any()):
        return reg.new_zeros(5)
    a, t, p, x = anchors[pos], tgt[pos], reg[pos], ctr[pos]
    tb = decode(t, a)
    acx, acy = (a[:, 0] + a[:, 2]) / 2, (a[:, 1] + a[:, 3]) / 2
    lr = torch.stack([acx - tb[:, 0], tb[:, 2] - acx], 1)
    tbm = torch.stack([acy - tb[:, 1], tb[:, 3] - acy], 1)
    ct = ((lr.min(1).values / lr.max(1).values) * (tbm.min(1).values / tbm.max(1).values)).sqrt()
    pb = decode(p, a)
    px2, py2 = torch.maximum(pb[:, 0], pb[:, 2]), torch.maximum(pb[:, 1], pb[:, 3])
    pa, ta = (px2 - pb[:, 0]) * (py2 - pb[:, 1]), (tb[:, 2] - tb[:, 0]) * (tb[:, 3] - tb[:, 1])
    ix1, iy1 = torch.maximum(pb[:, 0], tb[:, 0]), torch.maximum(pb[:, 1], tb[:, 1])
    ix2, iy2 = torch.minimum(px2, tb[:, 2]), torch.minimum(py2, tb[:, 3])
    inter = torch.where((ix2 > ix1) & (iy2 > iy1), (ix2 - ix1) * (iy2 - iy1), torch.zeros_like(ix1))
    enc = (torch.maximum(px2, tb[:, 2]) - torch.minimum(pb[:, 0], tb[:, 0])) * (torch.maximum(py2, tb[:, 3]) - torch.minimum(pb[:, 1], tb[:, 1])) + 1e-7
    union = pa + ta - inter + 1e-7
    gl = 1 - (inter / union - (enc - union) / enc)
    bce = x.clamp(min=0) - x * ct + torch.log1p(torch.exp(-x.abs()))
    return torch.stack([pos.sum().to(reg.dtype), ct.sum(), (gl * ct).sum(), bce.sum(), gl.sum()])


def token_targets_image(matched, pm, T):
    """[A, T] targets: the matched gt's positive-map row; background: 1 at the LAST column of the full map, 0 elsewhere"""
    A = matched.shape[0]
    tgt = torch.zeros(A, pm.shape[1], dtype=pm.dtype, device=matched.device)
    if pm.shape[0]:
        tgt = pm[matched.clamp(min=0)].clone()
    bg = matched < 0
    tgt[bg] = 0
    tgt[bg, -1] = 1
    return tgt[:, :T]


def token_loss_image(logits, tgt, mask, alpha, gamma):
    """summed binary focal loss over the live columns, in logits' dtype"""
    x, t = logits[:, mask > 0], tgt[:, mask > 0].to(logits.dtype)
    e = torch.exp(-x.abs())
    ce = x.clamp(min=0) - x * t + torch.log1p(e)
    p = torch.where(x >= 0, 1 / (1 + e), e / (1 + e))
    loss = ce * (1 - (p * t + (1 - p) * (1 - t))) ** gamma
    if alpha >= 0:
        loss = loss * (alpha * t + (1 - alpha) * (1 - t))
    return loss.sum()


def logits_of(tok, tk, tbias, dtype):
    """clamp(tok . tk^T + bias) in `dtype` from the operands as they are (already rounded to the kernel's operand type)"""
    return (torch.bmm(tok.to(dtype), tk.to(dtype).transpose(1, 2)) + tbias.to(dtype)[:, None, :]).clamp(-50000, 50000)


def losses_ref(levels, gts, labels, pms, reg, ctr, logits, mask, alpha, gamma, topk=9, reg_weight=2.0, token_weight=1.0, matched=None):
    """The whole objective for a batch, per-image loop -> dict (python floats in the dtype's precision) + matched list.  pms: per-image
    positive-map rows [G_b, Tfull]; logits [B, A, T]; mask [B, T]."""
    B = len(gts)
    sums = reg.new_zeros(5)
    tok = reg.new_zeros(())
    out_m = []
    for b in range(B):
        m = assign_image(levels, gts[b], topk) if matched is None else matched[b]
        out_m.append(m)
        sums = sums + box_sums_image(levels, gts[b], labels[b], m, reg[b], ctr[b])
        tgt = token_targets_image(m, pms[b].to(logits.device), logits.shape[2])
        tok = tok + token_loss_image(logits[b], tgt, mask[b], alpha, gamma)
    npos = max(float(sums[0]), 1.0)
    has = float(sums[0]) > 0
    giou = float(sums[2]) if float(sums[1]) > 0 else float(sums[4])
    return {"loss_reg": reg_weight * giou / float(sums[1]) if has else 0.0, "loss_centerness": float(sums[3]) / npos if has else 0.0,
            "loss_dot_product_token": token_weight * float(tok) / npos, "num_pos": int(sums[0]), "sums": [float(v) for v in sums] + [float(tok)],
            "matched": out_m}


# ------------------------------------------------------------------------------------------------ bit-stable draws
def head_draws(seed, B, A, T):
    """The random head outputs of a fixture case from INTEGER draws (bit-stable across numpy / platforms): every value is a small integer
    over a power of two, so it is exact in fp16, bf16 and fp32, and every 256-term dot product is exact in fp32 in any order.
    -> dict of float32 arrays: reg [B, A, 4] in [-2, 2], ctr [B, A] in [-4, 4], tok [B, A, 256] (k / 8), tk [B, T, 256] (k / 64),
    tbias [B, T] (k / 8 in [-3, 0]), cls [B, A] (the unused classification logits)."""
    rng = np.random.default_rng(seed)
    return {"reg": (rng.integers(-64, 65, (B, A, 4)) / 32.0).astype(np.float32),
            "ctr": (rng.integers(-64, 65, (B, A)) / 16.0).astype(np.float32),
            "tok": (rng.integers(-8, 9, (B, A, 256)) / 8.0).astype(np.float32),
            "tk": (rng.integers(-8, 9, (B, T, 256)) / 64.0).astype(np.float32),
            "tbias": (rng.integers(-24, 1, (B, T)) / 8.0).astype(np.float32),
            "cls": (rng.integers(-64, 1, (B, A)) / 16.0).astype(np.float32)}


def checksum(arrays):
    h = hashlib.sha256()
    for k in sorted(arrays):
        h.update(k.encode() + b"\0" + np.ascontiguousarray(arrays[k]).tobytes())
    return h.hexdigest()


def draw_boxes(rng, n, width, height, lo=12.0, hi=0.8, cluster=None):
    """n gt boxes with generic fractional corners inside a width x height canvas; `cluster` = (cx, cy, spread): centres near one point, so
    that the boxes overlap heavily and many anchors are claimed by several of them"""
    if cluster is None:
        cx, cy = rng.uniform(0.15, 0.85, n) * width, rng.uniform(0.15, 0.85, n) * height
    else:
        cx, cy = cluster[0] + rng.normal(0, cluster[2], n), cluster[1] + rng.normal(0, cluster[2], n)
    w, h = rng.uniform(lo, hi * width, n), rng.uniform(lo, hi * height, n)
    x1, y1 = np.clip(cx - w / 2, 0.37, width - 8), np.clip(cy - h / 2, 0.41, height - 8)
    x2, y2 = np.minimum(x1 + w, width - 1.13), np.minimum(y1 + h, height - 1.29)
    return np.stack([x1, y1, x2, y2], 1).astype(np.float32)
