"""TEST INFRASTRUCTURE ONLY: checks of the one match / accumulate kernel pair both AP evaluators launch (csrc/ap_eval.hip), at the level of
mq_det_amd.ops -- run through the kernel-source emulation by tests/test_ap_eval_cpu.py and on the device by tests/test_gpu_ap_eval.py.  The
inputs are hand-made; every expectation comes from the restatements tests/lvis_eval_ref.py / tests/coco_eval_ref.py, which the committed
fixtures pin to the references, never from the code under test."""
import numpy as np
import torch

import coco_eval_ref as cref
import lvis_eval_ref as lref

LVIS_FAST_GT, COCO_FAST_GT = 512, 256           # csrc/ap_eval.hip LvisRules / CocoRules fast_gt


class Case:
    """pairs: [(image index, category index, gts [(annotation id, [x, y, w, h], ignore / iscrowd)] in file order, dts [(score, [x, y, w, h])]
    score descending)] in (image, category) order, every pair with a ground truth or a detection; boxes and scores exact in fp32.
    ign_field: what the third entry of a ground truth is called in the json the restatements read."""

    def __init__(self, pairs, n_img, n_cat, ign_field="ignore"):
        assert [p[:2] for p in pairs] == sorted(p[:2] for p in pairs)
        self.pairs, self.K = pairs, n_cat
        cats = list(range(1, n_cat + 1))
        self.gt = {"images": [{"id": i + 1, "width": 1000, "height": 1000, "neg_category_ids": cats, "not_exhaustive_category_ids": []}
                              for i in range(n_img)],
                   "categories": [{"id": c, "name": str(c), "frequency": "f"} for c in cats],
                   "annotations": [{"id": aid, "image_id": i + 1, "category_id": c + 1, "bbox": box, "area": float(box[2] * box[3]), ign_field: int(ign)}
                                   for i, c, gts, _ in pairs for aid, box, ign in gts]}
        self.rows = np.asarray([[i + 1, c + 1, s] + box for i, c, _, dts in pairs for s, box in dts], np.float64).reshape(-1, 7)

    def tensors(self, dev):
        """what the evaluators hand to ops.*_match, and accumulate's per-category order, made here from the pairs"""
        t = lambda a, dt: torch.tensor(np.asarray(a), dtype=dt).to(dev)               # noqa: E731
        gts = [g for p in self.pairs for g in p[2]]
        nd = np.cumsum([0] + [len(p[3]) for p in self.pairs])
        ng = np.cumsum([0] + [len(p[2]) for p in self.pairs])
        out = {"pair_dt": t([[nd[n], len(p[3])] for n, p in enumerate(self.pairs)], torch.int32).reshape(-1, 2),
               "pair_gt": t([[ng[n], len(p[2])] for n, p in enumerate(self.pairs)], torch.int32).reshape(-1, 2),
               "pair_nel": torch.zeros(len(self.pairs), dtype=torch.uint8, device=dev),
               "dt_box": t(self.rows[:, 3:7], torch.float32).reshape(-1, 4),
               "gt_box": t([g[1] for g in gts], torch.float64).reshape(-1, 4),
               "gt_area": t([g[1][2] * g[1][3] for g in gts], torch.float64).reshape(-1),
               "gt_ign": t([int(g[2]) for g in gts], torch.uint8).reshape(-1),
               "gt_nz": t([int(g[0] != 0) for g in gts], torch.uint8).reshape(-1),
               "area_rng": t(lref.AREA_RNG, torch.float64), "iou_thr": t(lref.IOU_THRS, torch.float64), "rec_thr": t(lref.REC_THRS, torch.float64)}
        # accumulate: per category the detections in (image, position in the pair) order, stably sorted by descending score
        cat = np.concatenate([np.full(len(p[3]), p[1]) for p in self.pairs]).astype(np.int64)
        order = np.concatenate([np.nonzero(cat == k)[0][np.argsort(-self.rows[cat == k, 2], kind="stable")] for k in range(self.K)])
        out["order"] = t(order, torch.int32).reshape(-1)
        out["cat_off"] = t(np.cumsum([0] + [int((cat == k).sum()) for k in range(self.K)]), torch.int32)
        out["rank"] = t(np.concatenate([np.arange(len(p[3])) for p in self.pairs]), torch.int32).reshape(-1)
        return out

    def expected(self, rules):
        """-> (precision, recall, dt_bits [Nd, 2] uint64, gt_count [P, 4], num_gt [K, 4]) of the restatement"""
        if rules == "lvis":
            precision, recall, _, _, flags = lref.summarize_fixed(self.gt, self.rows, 1 << 20)
        else:
            e = cref.evaluate(self.gt, self.rows)
            precision, recall, flags = e["precision"], e["recall"], e["flags"]
        _, pc, _, bits, cnt = cref.pack_bits(flags, list(range(1, len(self.gt["images"]) + 1)), list(range(1, self.K + 1)))
        num_gt = np.zeros((self.K, 4), np.int64)
        np.add.at(num_gt, pc - 1, cnt)
        return precision, recall, bits, cnt, num_gt


def run(ops, rules, x, num_gt):
    """match + accumulate under one rule set -> (dt_bits as uint64, gt_count, precision, recall) as numpy arrays"""
    ng = torch.tensor(num_gt, dtype=torch.int32).to(x["dt_box"].device)
    if rules == "lvis":
        bits, cnt = ops.lvis_match(x["pair_dt"], x["pair_gt"], x["pair_nel"], x["dt_box"], x["gt_box"], x["gt_area"], x["gt_ign"], x["gt_nz"],
                                   x["area_rng"], x["iou_thr"])
        p, r = ops.lvis_accumulate(x["cat_off"], x["order"], bits, ng, x["rec_thr"])
    else:
        bits, cnt = ops.coco_match(x["pair_dt"], x["pair_gt"], x["dt_box"], x["gt_box"], x["gt_area"], x["gt_ign"], x["gt_nz"], x["area_rng"],
                                   x["iou_thr"])
        p, r = ops.coco_accumulate(x["cat_off"], x["order"], x["rank"], bits, ng, x["rec_thr"])
    return bits.cpu().numpy().view(np.uint64), cnt.cpu().numpy(), p.cpu().numpy(), r.cpu().numpy()


def check_rule_sets_coincide(ops, dev):
    """no crowd, no ignore, no not-exhaustive pair, at most 100 detections per pair: the two instantiations agree and equal the restatement.
    Two images x two categories: detections without ground truth, ground truths without detection, a pair in which one detection matches
    nothing (and one only a ground truth that is taken), one ground truth lies outside "small" and one annotation id is 0, a 1 x 1 pair."""
    pairs = [(0, 0, [], [(0.875, [30, 30, 20, 20]), (0.5625, [300, 300, 50, 50])]),
             (0, 1, [(1, [10, 10, 30, 30], 0), (2, [500, 500, 120, 120], 0)], []),
             (1, 0, [(5, [10, 10, 20, 20], 0), (6, [100, 100, 40, 40], 0), (0, [200, 200, 10, 10], 0)],
              [(0.9375, [10, 10, 20, 20]), (0.8125, [100, 100, 40, 30]), (0.75, [200, 200, 10, 10]), (0.625, [400, 400, 30, 30]),
               (0.5, [12, 10, 20, 20])]),
             (1, 1, [(7, [50, 50, 100, 100], 0)], [(0.6875, [55, 50, 100, 100])])]
    case = Case(pairs, 2, 2)
    want_p, want_r, want_bits, want_cnt, num_gt = case.expected("lvis")
    assert (want_bits[:, 0] != 0).any() and (want_bits[:, 0] == 0).any() and (want_p > 0).any() and (want_cnt[:, 1] != want_cnt[:, 0]).any()
    x = case.tensors(dev)
    lb, lc, lp, lr = run(ops, "lvis", x, num_gt)
    cb, cc, cp, cr = run(ops, "coco", x, num_gt)
    assert np.array_equal(lb, cb) and np.array_equal(lc, cc)
    assert np.array_equal(lp, cp[..., 2]) and np.array_equal(lr, cr[..., 2])
    assert np.array_equal(lb, want_bits) and np.array_equal(lc, want_cnt)
    assert np.array_equal(lp, want_p) and np.array_equal(lr, want_r)


def check_fast_path_bound(ops, dev, rules, n_gt):
    """one pair of 3 detections and n_gt ground truths on a grid, every 7th ignored (LVIS) / a crowd (COCO): the first detection lies on
    the last ground truth (index n_gt - 1: a plain one, except for n_gt = 512, where 511 = 7 * 73 is itself ignored), the other two on the
    same ignored / crowd one (a crowd takes both, an ignored one only the first)"""
    gts = [(n + 1, [float(n % 32 * 30), float(n // 32 * 30), 20.0, 20.0], n % 7 == 0) for n in range(n_gt)]
    on = lambda n, s: (s, [gts[n][1][0] + 1, gts[n][1][1], 20.0, 20.0])              # noqa: E731
    case = Case([(0, 0, gts, [on(n_gt - 1, 0.875), on(7, 0.75), on(7, 0.625)])], 1, 1, "ignore" if rules == "lvis" else "iscrowd")
    want_p, want_r, want_bits, want_cnt, num_gt = case.expected(rules)
    assert want_bits[0, 0] != 0 and want_bits[1, 1] != 0 and (want_bits[2, 0] != 0) == (rules == "coco")
    bits, cnt, p, r = run(ops, rules, case.tensors(dev), num_gt)
    assert np.array_equal(bits, want_bits) and np.array_equal(cnt, want_cnt)
    assert np.array_equal(p, want_p) and np.array_equal(r, want_r)


def check_max_dets_slices(ops, dev):
    """one category, one pair, 12 detections on 4 ground truths -- the detections of rank 0, 3, 6 and 10 each hit one, the others nothing --:
    the maxDets 1 / 10 / 100 slices of the COCO accumulate see 1, 3 and 4 true positives"""
    gts = [(n + 1, [100.0 * n, 0.0, 40.0, 40.0], 0) for n in range(4)]
    hit = {0: 0, 3: 1, 6: 2, 10: 3}
    dts = [(1 - n / 16, [100.0 * hit[n] if n in hit else 500.0 + 50 * n, 0.0, 40.0, 40.0]) for n in range(12)]
    case = Case([(0, 0, gts, dts)], 1, 1, "iscrowd")
    want_p, want_r, _, _, num_gt = case.expected("coco")
    assert not np.array_equal(want_p[..., 0], want_p[..., 1]) and not np.array_equal(want_p[..., 1], want_p[..., 2])
    _, _, p, r = run(ops, "coco", case.tensors(dev), num_gt)
    assert np.array_equal(p, want_p) and np.array_equal(r, want_r)
