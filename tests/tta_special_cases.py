"""Shared by tests/test_tta_special_cpu.py (kernel sources through tests/simt) and tests/test_gpu_tta_special.py (the MI355X): the seeded
detections, the cases and the comparison rules of the TEST.SPECIAL_NMS = 'soft-nms' / 'vote' / 'soft-vote' merges.

Shapes: B = 2 images of different size, T = 4 transforms (1 and 3 flipped, 3 with an area band), K = 40 slots with ragged counts, 147
live rows per image.  The class list (9, 2, 5, 3, 7, 1, 4) is out of order; 7 has no rows, 1 has one row, 4 two overlapping rows, 5
rows that all overlap (one cluster), 3 rows that never overlap, 9 and 2 random rows (9 has more than 32 per image: with the row cap
forced to 32 it takes the workspace path); labels 6 and 11 are outside the list; one score is NaN.  Scores are k / 4096, distinct."""
import numpy as np
import torch

import tta_special_ref as ref
from mq_det_amd import get_cfg

CLASSES = (9, 2, 5, 3, 7, 1, 4)
WH = [(64, 48), (40, 72)]                                  # original (w, h)
T, K = 4, 40
SCALE = (1.0, 1.0, 1.5, 1.5)
FLIP = (False, True, False, True)
RANGES = ((0, 10000), (0, 10000), (0, 10000), (8, 40))     # transform 3 keeps boxes of 64 .. 1600 px^2 (scaled frame) only
SEED = 5
INFERENCE_TH = 0.05
FORCED_CAP = 32
# (name, TEST.TH, TEST.PRE_NMS_TOP_N): the cut above and below the surviving count, and the pass-through
CASES = {"soft-nms": (("nocut", 0.3, 1000), ("cut", 0.3, 25), ("through", 0.0, 1000)),
         "vote": (("nocut", 0.5, 1000), ("cut", 0.5, 25), ("through", 0.0, 1000)),
         "soft-vote": (("nocut", 0.5, 1000), ("cut", 0.5, 25), ("through", 0.0, 1000))}


def _orig_rows(g, w, h):
    """Rows of one image in its original frame: (box, label) lists per kind."""
    rows = []
    for lab, n in ((9, 64), (2, 36), (6, 8), (11, 6)):                       # random rows; 6 and 11 are not in the class list
        x1, y1 = g.uniform(0, 0.6 * w, n), g.uniform(0, 0.6 * h, n)
        for i in range(n):
            rows.append(([x1[i], y1[i], x1[i] + g.uniform(4, 0.4 * w), y1[i] + g.uniform(4, 0.4 * h)], lab))
    for i in range(14):                                                       # class 5: one box, jittered: every pair overlaps
        j = g.uniform(-0.6, 0.6, 4)
        rows.append(([0.2 * w + j[0], 0.2 * h + j[1], 0.7 * w + j[2], 0.7 * h + j[3]], 5))
    for i in range(16):                                                       # class 3: a grid of small boxes with gaps
        cx, cy = (i % 4) * 0.22 * w + 2, (i // 4) * 0.22 * h + 2
        rows.append(([cx, cy, cx + 0.1 * w, cy + 0.1 * h], 3))
    rows.append(([0.1 * w, 0.1 * h, 0.5 * w, 0.5 * h], 1))                    # class 1: one row
    rows.append(([0.3 * w, 0.3 * h, 0.8 * w, 0.8 * h], 4))                    # class 4: two rows, IoU about 0.8
    rows.append(([0.3 * w + 2, 0.3 * h + 1, 0.8 * w + 1, 0.8 * h + 2], 4))
    return rows


def build_dets(seed=SEED):
    """-> dets for tta.merge (host tensors): per transform (packed [B, K, 6], counts, scaled (w, h), flipped, range)."""
    g = np.random.default_rng(seed)
    B = len(WH)
    pool = g.permutation(np.arange(1, 4000)).astype(np.float32) / np.float32(4096.0)
    packed = np.zeros((T, B, K, 6), np.float32)
    counts = np.zeros((T, B), np.int64)
    used = 0
    for b, (w, h) in enumerate(WH):
        rows = _orig_rows(g, w, h)
        order = np.concatenate([np.arange(len(rows) - 3, len(rows)), g.permutation(len(rows) - 3)])   # classes 1 and 4: never in the banded transform
        cut = np.cumsum([38 - 3 * b, 31 + 2 * b, 40])       # ragged counts, one transform full
        assert 0 < len(rows) - cut[-1] <= K
        for t, part in enumerate(np.split(order, cut)):
            s = SCALE[t]
            ws = int(w * s)
            bx = np.array([rows[i][0] for i in part], np.float64) * s
            if FLIP[t]:                                      # into the flipped frame: the merge flips it back
                bx = np.stack([ws - bx[:, 2] - 1, bx[:, 1], ws - bx[:, 0] - 1, bx[:, 3]], 1)
            sc = pool[used:used + len(part)].copy()
            used += len(part)
            if b == 0 and t == 2:
                sc[3] = np.nan
            o = np.argsort(-np.nan_to_num(sc, nan=2.0), kind="stable")       # score-sorted like the model's rows
            packed[t, b, :len(part)] = np.concatenate([bx[o], sc[o, None], np.array([rows[i][1] for i in part], np.float64)[o, None]], 1)
            counts[t, b] = len(part)
    dets = []
    for t in range(T):
        wh = [(int(w * SCALE[t]), int(h * SCALE[t])) for (w, h) in WH]
        dets.append((torch.from_numpy(packed[t]), [int(c) for c in counts[t]], wh, FLIP[t], RANGES[t]))
    return dets


def make_cfg(mode, th, top_n):
    cfg = get_cfg()
    cfg.TEST.SPECIAL_NMS, cfg.TEST.TH, cfg.TEST.PRE_NMS_TOP_N, cfg.TEST.SELECT_CLASSES = mode, th, top_n, CLASSES
    cfg.MODEL.RETINANET.INFERENCE_TH = INFERENCE_TH
    return cfg


def prep_restated(dets, orig_wh):
    """The rows the merge works on, per image: un-flip, area band, rescale, concatenated in transform order (box_aug.py:21-63) ->
    [(boxes [n, 4] fp32, scores, labels int64) numpy]."""
    out = []
    for b, (w, h) in enumerate(orig_wh):
        B_, S_, L_ = [], [], []
        for packed, counts, wh, fl, rng in dets:
            p = packed[b, :counts[b]]
            bx, sc, lb = p[:, :4].clone(), p[:, 4].clone(), p[:, 5].to(torch.int64)
            ws, hs = wh[b]
            if fl:
                bx = torch.stack([ws - bx[:, 2] - 1, bx[:, 1], ws - bx[:, 0] - 1, bx[:, 3]], 1)
            if rng is not None:
                ar = (bx[:, 2] - bx[:, 0] + 1) * (bx[:, 3] - bx[:, 1] + 1)
                k = (ar > rng[0] * rng[0]) & (ar < rng[1] * rng[1])
                bx, sc, lb = bx[k], sc[k], lb[k]
            rw, rh = float(w) / float(ws), float(h) / float(hs)
            B_.append(bx * torch.tensor([rw, rh, rw, rh], dtype=torch.float32)), S_.append(sc), L_.append(lb)
        out.append((torch.cat(B_).numpy(), torch.cat(S_).numpy(), torch.cat(L_).numpy()))
    return out


_WANT = {}


def expected(mode, th, top_n):
    """The restated reference on the shared rows, computed once per case and never modified."""
    key = (mode, th, top_n)
    if key not in _WANT:
        rows = prep_restated(build_dets(), WH)
        _WANT[key] = [ref.merge_special(bx, sc, lb, CLASSES, mode, th, INFERENCE_TH, top_n) for bx, sc, lb in rows]
    return _WANT[key]


def check_conditions(mode, th, want):
    """What the comparison rules rest on, asserted from the margins the restated reference met."""
    for w in want:
        m = w["margins"]
        assert m["in_distinct"], "input scores repeat inside a class"
        assert m["out_distinct"], "output scores repeat inside a class"
        if mode == "soft-nms" and th > 0:
            bound = (m["max_decays"] + 1) * 2.0 ** -23
            assert m["thr_gap"] >= 2 * bound, (m["thr_gap"], bound)
            assert m["pick_gap"] >= 2 * bound, (m["pick_gap"], bound)


def compare(mode, th, got, want, where=""):
    """got: list[BoxList] (host), want: expected(...).  Counts, labels and order exact; then per mode:
      vote / soft-vote  scores exact, boxes exact except the weighted means: |d| <= (m + 3) 2^-24 max|coord| of the cluster
                        (the reference's sequential fp32 sum carries m + 2 roundings, a sum in any order or in fp64 at most one more)
      soft-nms          boxes exact, scores within (k + 1) 2^-23 relative after k decays (one fp32 rounding per decay, and the fp64 factor
                        may differ from libm's in its last place, which moves the rounded product by at most one more fp32 ulp)."""
    assert [len(r) for r in got] == [len(w["scores"]) for w in want], where
    for b, (r, w) in enumerate(zip(got, want)):
        gb, gs, gl = r.bbox.numpy(), r.get_field("scores").numpy(), r.get_field("labels").numpy()
        assert gl.dtype == np.int64 and np.array_equal(gl, w["labels"]), (where, b)
        if th <= 0:
            assert np.array_equal(gb, w["boxes"]) and np.array_equal(gs, w["scores"]), (where, b)
        elif mode == "soft-nms":
            assert np.array_equal(gb, w["boxes"]), (where, b)
            tol = (w["decays"] + 1) * 2.0 ** -23 * np.abs(w["scores"].astype(np.float64))
            err = np.abs(gs.astype(np.float64) - w["scores"].astype(np.float64))
            assert (err <= tol).all(), (where, b, float((err / np.maximum(tol, 1e-300)).max()))
            assert np.array_equal(gs[w["decays"] == 0], w["scores"][w["decays"] == 0]), (where, b)
        else:
            assert np.array_equal(gs, w["scores"]), (where, b)
            plain = w["avg"] == 0
            assert np.array_equal(gb[plain], w["boxes"][plain]), (where, b)
            tol = ((w["avg"] + 3) * 2.0 ** -24 * w["cmax"])[:, None]
            err = np.abs(gb.astype(np.float64) - w["boxes"].astype(np.float64))
            assert (err[~plain] <= tol[~plain]).all(), (where, b, float((err[~plain] / tol[~plain]).max()))


def to_device(dets, device):
    return [(d[0].to(device),) + tuple(d[1:]) for d in dets]


def host(res):
    from mq_det_amd.structures import BoxList
    out = []
    for r in res:
        bl = BoxList(r.bbox.cpu(), r.size, mode=r.mode)
        for f in r.fields():
            bl.add_field(f, r.get_field(f).cpu())
        out.append(bl)
    return out
