"""A from-scratch restatement of MQ-GroundingDINO's set criterion (matcher.py HungarianMatcher, loss.py SetCriterion) in numpy / torch: the
matching cost, a plain sequential rectangular linear-sum-assignment solver (shortest augmenting paths, Crouse 2016) and the loss sums.  It is
checked against scipy and the recorded reference (tests/golden/set_loss) in the CPU suite and is the yardstick where scipy is absent."""
import math

import numpy as np
import torch

GAMMA = 2.0


def class_term(logits, alpha):
    """pos_cost_class - neg_cost_class per (query, token), matcher.py:52-64, in the dtype of `logits`"""
    p = logits.sigmoid()
    neg = (1 - alpha) * (p ** GAMMA) * (-(1 - p + 1e-8).log())
    pos = alpha * ((1 - p) ** GAMMA) * (-(p + 1e-8).log())
    return pos - neg


def xyxy(b):
    cx, cy, w, h = b.unbind(-1)
    return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)


def giou_matrix(a, g):
    """util/box_ops.py generalized_box_iou of xyxy boxes [N, 4] x [M, 4] -> [N, M]"""
    area1 = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area2 = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
    wh = (torch.min(a[:, None, 2:], g[:, 2:]) - torch.max(a[:, None, :2], g[:, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    union = area1[:, None] + area2 - inter
    wh = (torch.max(a[:, None, 2:], g[:, 2:]) - torch.min(a[:, None, :2], g[:, :2])).clamp(min=0)
    enc = wh[..., 0] * wh[..., 1]
    return inter / (union + 1e-6) - (enc - union) / (enc + 1e-6)


def cost_ref(logits, boxes, gts, posmaps, wc=1.0, wb=5.0, wg=2.0, alpha=0.25, dtype=torch.float64):
    """logits [B, nq, T] (-inf at padded positions), boxes [B, nq, 4] cxcywh; per image gts [G, 4] and posmaps [G, Tpm] -> per image the
    gt-major cost [G, nq].  A positive token at a column >= T has p = 0."""
    out = []
    for b in range(logits.shape[0]):
        x, pm = logits[b].to(dtype), posmaps[b]
        if pm.shape[1] > x.shape[1]:
            x = torch.cat([x, x.new_full((x.shape[0], pm.shape[1] - x.shape[1]), -math.inf)], 1)
        d = class_term(x, alpha)
        bx, g = boxes[b].to(dtype), gts[b].to(dtype)
        cls = torch.stack([d[:, row > 0].mean(-1) for row in pm]) if len(pm) else d.new_zeros(0, x.shape[0])
        l1 = (g[:, None, :] - bx[None, :, :]).abs().sum(-1)
        out.append(wb * l1 + wc * cls - wg * giou_matrix(xyxy(bx), xyxy(g)).t() if len(g) else d.new_zeros(0, x.shape[0]))
    return out


def lsap(cost):
    """Minimum-cost assignment of a [G, n] matrix, G <= n, every row assigned: -> col4row [G] int64.  Shortest augmenting paths with fp64
    duals; an argmin tie goes to the lower column."""
    C = np.asarray(cost, dtype=np.float64)
    G, n = C.shape
    assert G <= n
    if not np.isfinite(C).all():
        raise ValueError("lsap: non-finite cost")
    u, v = np.zeros(G), np.zeros(n)
    col4row, row4col = np.full(G, -1, np.int64), np.full(n, -1, np.int64)
    for cur in range(G):
        shortest = np.full(n, np.inf)
        path = np.full(n, -1, np.int64)
        in_tree = np.zeros(n, bool)
        rows_in_tree = []
        minval, i, sink = 0.0, cur, -1
        for _ in range(cur + 1):
            rows_in_tree.append(i)
            r = minval + C[i] - u[i] - v
            better = ~in_tree & (r < shortest)
            shortest[better] = r[better]
            path[better] = i
            masked = np.where(in_tree, np.inf, shortest)
            j = int(np.argmin(masked))                           # numpy: the first (lowest) index of the minimum
            minval = masked[j]
            assert np.isfinite(minval)
            in_tree[j] = True
            if row4col[j] < 0:
                sink = j
                break
            i = row4col[j]
        assert sink >= 0
        u[cur] += minval
        for i in rows_in_tree[1:]:
            u[i] += minval - shortest[col4row[i]]
        v[in_tree] -= minval - shortest[in_tree]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    return col4row


def total(cost, col4row):
    C = np.asarray(cost, dtype=np.float64)
    return float(C[np.arange(len(col4row)), np.asarray(col4row)].sum())


def gap_to_second_best(cost, solve=lsap):
    """cost of the best assignment that differs from the optimum, minus the optimum (forbid each matched pair in turn, re-solve)"""
    C = np.asarray(cost, dtype=np.float64)
    best = solve(C)
    opt = total(C, best)
    big = np.abs(C).max() * (len(C) + 1) + 1.0
    gap = np.inf
    for r, c in enumerate(best):
        D = C.copy()
        D[r, c] = big
        gap = min(gap, total(D, solve(D)) - opt)
    return gap


def indices_of(col4row):
    """the reference's (index_i, index_j): query indices ascending and the gt of each"""
    col4row = torch.as_tensor(np.asarray(col4row), dtype=torch.int64)
    order = torch.argsort(col4row)
    return col4row[order], order


def focal_sum(x, t, alpha, gamma):
    """token_sigmoid_binary_focal_loss summed (layers/sigmoid_focal_loss.py:130-171)"""
    p = torch.sigmoid(x)
    ce = torch.nn.functional.binary_cross_entropy_with_logits(x, t, reduction="none")
    loss = ce * (1 - (p * t + (1 - p) * (1 - t))) ** gamma
    if alpha >= 0:
        loss = (alpha * t + (1 - alpha) * (1 - t)) * loss
    return loss.sum()


def sums_ref(logits, boxes, gts, posmaps, text_mask, indices, alpha=0.25, gamma=2.0, dtype=torch.float64):
    """loss_labels / loss_boxes of one layer as raw sums (loss.py:42-91): logits [B, nq, T], text_mask [B, T], indices per image (index_i,
    index_j) -> (token focal sum, S |src - tgt|, S (1 - GIoU))"""
    B, nq, T = logits.shape
    Tpm = posmaps[0].shape[1]
    tok = l1 = gi = 0.0
    for b in range(B):
        tgt = torch.zeros(nq, Tpm, dtype=dtype)
        qi, gj = indices[b]
        tgt[qi] = (posmaps[b][gj] > 0).to(dtype)
        tgt[tgt.sum(-1) == 0, -1] = 1.0
        live = text_mask[b, :T] > 0
        tok += float(focal_sum(logits[b].to(dtype)[:, live], tgt[:, :T][:, live], alpha, gamma))
        if len(qi):
            src, g = boxes[b].to(dtype)[qi], gts[b].to(dtype)[gj]
            l1 += float((src - g).abs().sum())
            gi += float((1 - torch.diag(giou_matrix(xyxy(src), xyxy(g)))).sum())
    return tok, l1, gi


def losses_from_sums(sums, num_boxes, coef=(2.0, 5.0, 2.0)):
    """the reference's dict from per-layer sums [L, 3]: the last layer is the main output, the others are aux 0 .. L - 2"""
    out = {}
    L = len(sums)
    for l in range(L):
        sfx = "" if l == L - 1 else f"_{l}"
        for name, c, s in zip(("loss_ce", "loss_bbox", "loss_giou"), coef, sums[l]):
            out[name + sfx] = float(s) / num_boxes * c
    return out
