"""TEST REFERENCE ONLY: TEST.SPECIAL_NMS = 'soft-nms' / 'vote' / 'soft-vote' of the reference's multi-scale merge, restated in numpy.

  soft_nms         csrc/cpu/soft_nms.cpp as box_aug.py calls it (threshold = TEST.TH on the SCORE, sigma = 0.95): fp32 areas and IoU with
                   the legacy +1, the decay factor exp(-ovr^2 / sigma) in fp64, the product rounded to fp32 on the store, the first
                   maximum taken at every pick, a discarded row replaced by the last one (which is then looked at in its place).
  bbox_vote        box_aug.py:241-287 and
  soft_bbox_vote   box_aug.py:290-349, every operation on float32 arrays exactly as numpy evaluates it (sums included).
  merge_special    the per-class loop and the top-N cut around them (box_aug.py:166-206, boxlist_nms), on rows that are already in the
                   original frame.

Besides the rows every function returns what a test needs to hold another implementation to them: per output row how it was made
(`avg` = cluster size when the box is a weighted mean, else 0; `cmax` = the largest |coordinate| in that cluster; `decays` = the number
of soft-NMS decays the score received) and the MARGINS met on the way (soft-NMS: the smallest |s - threshold| relative to s at any check,
the smallest relative gap between the best and the second-best score at any pick, the largest number of decays any row received; all modes: whether scores are pairwise distinct).
PER-ROW MARGINS (the random-shape sweep, tests/tta_special_draws.py): a decay is EFFECTIVE when ovr > 0 -- a factor of exactly 1 rounds nothing
on either side -- and a score that received e effective decays is known to (e + 1) 2^-23 relative (the argument of tta_special_cases.compare).
  thr_ratio   min over every threshold comparison of |s - threshold| / |s| divided by the row's own bound (e + 1) 2^-23
  pick_ratio  min over every pick of the relative gap between the best and the second-best live score divided by (e_best + e_second + 1) 2^-23
  cut_ratio   the same for the two scores on either side of the top-N cut actually used (soft-nms only: the voting modes' scores are exact,
              a tie at the cut is legal there and is compared exactly)
A ratio below 2 means another correct implementation may decide the other way: such a draw is not run.  `eff` per output row goes with them.
tools/gen_golden_tta_special.py pins these restatements against the reference's own functions (tests/golden/tta_special)."""
import numpy as np

F = np.float32
SIGMA = 0.95
MODES = ("soft-nms", "vote", "soft-vote")


def _distinct(v):
    v = np.asarray(v)
    return len(np.unique(v)) == len(v)


ULP = 2.0 ** -23


def soft_nms(boxes, scores, threshold, sigma=SIGMA, margins=None, with_eff=False):
    """-> (kept original indices in pick order, their decayed fp32 scores, decays received per kept row[, effective decays per kept row])."""
    boxes, s = np.asarray(boxes, F).reshape(-1, 4), np.array(scores, F).reshape(-1)
    n = len(s)
    if n == 0:
        return (np.zeros(0, np.int64), np.zeros(0, F), np.zeros(0, np.int64)) + ((np.zeros(0, np.int64),) if with_eff else ())
    x1, y1, x2, y2 = (boxes[:, c].copy() for c in range(4))
    area = (x2 - x1 + F(1)) * (y2 - y1 + F(1))
    ind, dec, eff = np.arange(n), np.zeros(n, np.int64), np.zeros(n, np.int64)
    thr, sig = F(threshold), np.float64(F(sigma))
    cols = (x1, y1, x2, y2, s, area, ind, dec, eff)
    i = 0
    while i < n:
        live = s[i:n]
        p = int(np.argmax(live)) + i                          # the first maximum, like at::argmax
        if margins is not None and n - i > 1:
            two = np.sort(live)[-2:]
            margins["pick_gap"] = min(margins["pick_gap"], float((two[1] - two[0]) / abs(two[1])))
            a2 = np.argpartition(live, -2)[-2:]                # the two rows compared: their own bound
            gap = abs(float(live[a2[1]]) - float(live[a2[0]])) / abs(float(two[1]))
            margins["pick_ratio"] = min(margins.get("pick_ratio", np.inf), gap / ((int(eff[i + a2[0]]) + int(eff[i + a2[1]]) + 1) * ULP))
        for c in cols:
            c[i], c[p] = c[p], c[i]
        if n - i > 1:
            j = slice(i + 1, n)
            w = np.maximum(F(0), np.minimum(x2[i], x2[j]) - np.maximum(x1[i], x1[j]) + F(1))
            h = np.maximum(F(0), np.minimum(y2[i], y2[j]) - np.maximum(y1[i], y1[j]) + F(1))
            inter = w * h
            ovr = inter / (area[i] + area[j] - inter)
            assert ovr.dtype == F
            s[j] = (s[j].astype(np.float64) * np.exp(-(ovr.astype(np.float64) ** 2) / sig)).astype(F)
            dec[j] += 1
            eff[j] += ovr > 0
            if margins is not None:
                margins["max_decays"] = max(margins["max_decays"], int(dec[j].max()))
                rel = np.abs(s[j].astype(np.float64) - np.float64(thr)) / np.abs(s[j].astype(np.float64))
                margins["thr_gap"] = min(margins["thr_gap"], float(np.min(np.abs(s[j] - thr) / np.abs(s[j]))))
                margins["thr_ratio"] = min(margins.get("thr_ratio", np.inf), float(np.min(rel / ((eff[j] + 1) * ULP))))
            k = i + 1
            while k < n:                                      # discard: the last row takes the place and is checked there
                if s[k] < thr:
                    for c in cols:
                        c[k] = c[n - 1]
                    n -= 1
                else:
                    k += 1
        i += 1
    return (ind[:n].copy(), s[:n].copy(), dec[:n].copy()) + ((eff[:n].copy(),) if with_eff else ())


def _vote(boxes, scores, vote_thresh, soft_thresh):
    """bbox_vote (soft_thresh None) / soft_bbox_vote -> (rows [n, 5] float64 as the reference stacks them, avg, cmax) or None for a
    class of fewer than two rows (the caller then leaves the class untouched)."""
    det = np.concatenate((np.asarray(boxes, F).reshape(-1, 4), np.asarray(scores, F).reshape(-1, 1)), axis=1)
    assert det.dtype == F
    if det.shape[0] <= 1:
        return None
    det = det[det[:, 4].ravel().argsort()[::-1], :]
    rows, avg, cmax = [], [], []
    while det.shape[0] > 0:
        area = (det[:, 2] - det[:, 0] + 1) * (det[:, 3] - det[:, 1] + 1)
        w = np.maximum(0.0, np.minimum(det[0, 2], det[:, 2]) - np.maximum(det[0, 0], det[:, 0]) + 1)
        h = np.maximum(0.0, np.minimum(det[0, 3], det[:, 3]) - np.maximum(det[0, 1], det[:, 1]) + 1)
        inter = w * h
        o = inter / (area[0] + area[:] - inter)
        assert o.dtype == F
        idx = np.where(o >= vote_thresh)[0]
        acc, acc_o = det[idx, :], o[idx]
        det = np.delete(det, idx, 0)
        if idx.shape[0] <= 1:
            rows.append(acc.astype(np.float64))
            avg += [0] * len(acc)
            cmax += [0.0] * len(acc)
            continue
        big = float(np.abs(acc[:, :4]).max())
        extra = None
        if soft_thresh is not None:
            soft = acc.copy()
            soft[:, 4] = soft[:, 4] * (1 - acc_o)
            extra = soft[np.where(soft[:, 4] >= soft_thresh)[0], :]
        acc[:, 0:4] = acc[:, 0:4] * np.tile(acc[:, -1:], (1, 4))
        one = np.zeros((1, 5))
        one[:, 0:4] = np.sum(acc[:, 0:4], axis=0) / np.sum(acc[:, -1:])
        one[:, 4] = np.max(acc[:, 4])
        rows.append(one)
        avg.append(len(idx))
        cmax.append(big)
        if extra is not None and extra.shape[0] > 0:
            rows.append(extra.astype(np.float64))
            avg += [0] * len(extra)
            cmax += [0.0] * len(extra)
    rows, avg, cmax = np.concatenate(rows, 0), np.asarray(avg), np.asarray(cmax)
    if soft_thresh is not None:
        order = rows[:, 4].ravel().argsort()[::-1]
        rows, avg, cmax = rows[order, :], avg[order], cmax[order]
    return rows, avg, cmax


def bbox_vote(boxes, scores, vote_thresh):
    return _vote(boxes, scores, vote_thresh, None)


def soft_bbox_vote(boxes, scores, vote_thresh, soft_thresh):
    return _vote(boxes, scores, vote_thresh, soft_thresh)


def merge_classes(boxes, scores, labels, class_list, mode, th, inference_th):
    """The per-class loop of merge_special before the top-N cut -> (columns [boxes, scores, labels, avg, cmax, decays, eff], margins)."""
    boxes, scores, labels = np.asarray(boxes, F).reshape(-1, 4), np.asarray(scores, F).reshape(-1), np.asarray(labels).reshape(-1)
    ok = ~np.isnan(scores)
    boxes, scores, labels = boxes[ok], scores[ok], labels[ok]
    margins = {"thr_gap": np.inf, "pick_gap": np.inf, "max_decays": 0, "in_distinct": True, "out_distinct": True,
               "thr_ratio": np.inf, "pick_ratio": np.inf, "cut_ratio": np.inf}
    B_, S_, L_, A_, C_, D_, E_ = [], [], [], [], [], [], []
    for j in class_list:
        i = np.nonzero(labels == j)[0]
        b, s = boxes[i], scores[i]
        margins["in_distinct"] &= _distinct(s)
        avg, cmax, dec = np.zeros(len(s), np.int64), np.zeros(len(s)), np.zeros(len(s), np.int64)
        eff = np.zeros(len(s), np.int64)
        if th > 0 and mode == "soft-nms":
            keep, s, dec, eff = soft_nms(b, s, th, SIGMA, margins, with_eff=True)
            b, avg, cmax = b[keep], avg[keep], cmax[keep]
        elif th > 0 and mode in ("vote", "soft-vote"):
            r = bbox_vote(b, s, th) if mode == "vote" else soft_bbox_vote(b, s, th, inference_th)
            if r is not None:                                 # (fewer than two rows: len(boxes_vote) == 0, the class is left as it is)
                b, s, avg, cmax = r[0][:, :4].astype(F), r[0][:, 4].astype(F), r[1], r[2]
                dec = np.zeros(len(s), np.int64)
                eff = np.zeros(len(s), np.int64)
        elif th > 0:
            raise ValueError(mode)
        margins["out_distinct"] &= _distinct(s)
        B_.append(b), S_.append(s), L_.append(np.full(len(s), j, np.int64)), A_.append(avg), C_.append(cmax), D_.append(dec), E_.append(eff)
    return [np.concatenate(v) if len(v) else np.zeros(0) for v in (B_, S_, L_, A_, C_, D_, E_)], margins


def cut_top_n(cols, margins, top_n):
    """kthvalue(scores, n - top_n + 1), keep >= (box_aug.py:199-206) on the columns of merge_classes -> the dict of merge_special."""
    out, margins = list(cols), dict(margins)
    n = len(out[1])
    if n > top_n > 0:
        order = np.argsort(out[1], kind="stable")
        kth = out[1][order[n - top_n]]                        # kthvalue(scores, n - top_n + 1)
        lo, hi = order[n - top_n - 1], order[n - top_n]       # the two scores on either side of the cut
        gap = abs(float(out[1][hi]) - float(out[1][lo])) / abs(float(out[1][hi]))
        margins["cut_ratio"] = gap / ((int(out[6][lo]) + int(out[6][hi]) + 1) * ULP)
        k = out[1] >= kth
        out = [v[k] for v in out]
    return {"boxes": out[0].reshape(-1, 4).astype(F), "scores": out[1].astype(F), "labels": out[2].astype(np.int64), "avg": out[3].astype(np.int64),
            "cmax": out[4].astype(np.float64), "decays": out[5].astype(np.int64), "eff": out[6].astype(np.int64), "margins": margins}


def merge_special(boxes, scores, labels, class_list, mode, th, inference_th, top_n):
    """One image: rows in the original frame (fp32 boxes [n, 4], fp32 scores, int labels) -> dict(boxes fp32, scores fp32, labels int64,
    avg, cmax, decays, eff per output row, margins).  A NaN score is dropped first, as the device merge does."""
    cols, margins = merge_classes(boxes, scores, labels, class_list, mode, th, inference_th)
    return cut_top_n(cols, margins, top_n)
