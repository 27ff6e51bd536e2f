"""Shared by tests/test_tta_candidates_cpu.py (kernel sources through tests/simt) and tests/test_gpu_tta_candidates.py (the MI355X): the
restated merge, the seeded draws and the comparison of the per-class NMS at any row count (mq_tta_merge_nms, csrc/tta.hip), the NMS of the
TEST.SPECIAL_NMS = 'none' merge when TEST.USE_MULTISCALE hands it every transform's un-suppressed candidates.

`merge_restated` follows box_aug.py:21-63 and :150-206 on numpy arrays in fp32, operation by operation: un-flip (BoxList.transpose),
remove_boxes, BoxList.resize, concatenation in transform order, then per class of the class list (in ITS order) _C.nms -- score order,
greedy, IoU > TEST.TH with the legacy +1, kept rows in their original order --, then the kthvalue cut at TEST.PRE_NMS_TOP_N with ties kept.
What the device merge states beyond the reference (include/mqdet_hip.h): a NaN score is dropped (it has no place in a total order), a
label outside the class list is dropped (as the reference's per-class loop never visits it), equal scores go to the lower row.

The toy draws (T <= 4, B <= 3, K <= 200) are sized for the emulator and for ROW_CAP = 8, at which the workspace path of the kernel runs."""
import numpy as np
import torch

from mq_det_amd import get_cfg, tta

ROW_CAP = 8
F = np.float32


def prep_restated(dets, orig_wh):
    """-> per image (boxes [n, 4] fp32, scores [n] fp32, labels [n] int64): the rows box_aug.py concatenates, NaN scores dropped."""
    out = []
    for b, (w, h) in enumerate(orig_wh):
        B_, S_, L_ = [], [], []
        for packed, counts, wh, fl, rng in dets:
            p = packed[b, :counts[b]].cpu().numpy().astype(F)
            bx, sc, lb = p[:, :4].copy(), p[:, 4].copy(), p[:, 5].astype(np.int64)
            ws, hs = wh[b]
            if fl:                                           # BoxList.transpose(FLIP_LEFT_RIGHT), TO_REMOVE = 1
                bx = np.stack([(F(ws) - bx[:, 2]) - F(1), bx[:, 1], (F(ws) - bx[:, 0]) - F(1), bx[:, 3]], 1)
            if rng is not None:                              # remove_boxes
                ar = (bx[:, 2] - bx[:, 0] + F(1)) * (bx[:, 3] - bx[:, 1] + F(1))
                k = (ar > F(rng[0] * rng[0])) & (ar < F(rng[1] * rng[1]))
                bx, sc, lb = bx[k], sc[k], lb[k]
            rw, rh = F(float(w) / float(ws)), F(float(h) / float(hs))
            bx = bx * np.array([rw, rh, rw, rh], F)
            ok = ~np.isnan(sc)
            B_.append(bx[ok]), S_.append(sc[ok]), L_.append(lb[ok])
        out.append((np.concatenate(B_), np.concatenate(S_), np.concatenate(L_)))
    return out


def nms_restated(bx, sc, thresh):
    """_C.nms (csrc/cuda/nms.cu): rows in (score descending, row ascending) order, greedy, IoU > thresh with the +1 -> kept rows ascending."""
    n = len(sc)
    order = np.argsort(-sc, kind="stable")
    b = bx[order]
    area = (b[:, 2] - b[:, 0] + F(1)) * (b[:, 3] - b[:, 1] + F(1))
    removed = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if removed[i]:
            continue
        keep.append(order[i])
        r = b[i + 1:]
        w = np.maximum(np.minimum(b[i, 2], r[:, 2]) - np.maximum(b[i, 0], r[:, 0]) + F(1), F(0))
        h = np.maximum(np.minimum(b[i, 3], r[:, 3]) - np.maximum(b[i, 1], r[:, 1]) + F(1), F(0))
        inter = w * h
        removed[i + 1:] |= inter / (area[i] + area[i + 1:] - inter) > F(thresh)
    return np.sort(np.asarray(keep, np.int64))


def merge_restated(dets, orig_wh, cfg):
    """-> per image (boxes, scores, labels int64) numpy: merge_result_from_multi_scales with SPECIAL_NMS 'none' on the rows of `dets`."""
    out = []
    th, top = float(cfg.TEST.TH), int(cfg.TEST.PRE_NMS_TOP_N)
    for bx, sc, lb in prep_restated(dets, orig_wh):
        rb, rs, rl = [np.zeros((0, 4), F)], [np.zeros(0, F)], [np.zeros(0, np.int64)]
        for j in tta.class_list(cfg):
            i = np.nonzero(lb == j)[0]
            keep = nms_restated(bx[i], sc[i], th) if th > 0 else np.arange(len(i))
            rb.append(bx[i][keep]), rs.append(sc[i][keep]), rl.append(np.full(len(keep), j, np.int64))
        rb, rs, rl = np.concatenate(rb), np.concatenate(rs), np.concatenate(rl)
        n = len(rs)
        if n > top > 0:
            thr = np.sort(rs)[n - top]                        # torch.kthvalue(scores, n - top + 1)
            k = rs >= thr
            rb, rs, rl = rb[k], rs[k], rl[k]
        out.append((rb, rs, rl))
    return out


def compare_exact(got, want, where=""):
    """got: list[BoxList]; want: merge_restated(...).  Counts, boxes, scores and labels bit for bit."""
    assert [len(r) for r in got] == [len(w[1]) for w in want], where
    for b, (r, (rb, rs, rl)) in enumerate(zip(got, want)):
        lab = r.get_field("labels").cpu()
        assert lab.dtype == torch.int64
        assert np.array_equal(r.bbox.cpu().numpy(), rb), (where, b)
        assert np.array_equal(r.get_field("scores").cpu().numpy(), rs), (where, b)
        assert np.array_equal(lab.numpy(), rl), (where, b)


def same_boxlists(a, b):
    return len(a) == len(b) and all(torch.equal(x.bbox, y.bbox) and torch.equal(x.get_field("scores"), y.get_field("scores"))
                                    and torch.equal(x.get_field("labels"), y.get_field("labels")) for x, y in zip(a, b))


def make_cfg(classes, th=0.5, top_n=1000):
    cfg = get_cfg()
    cfg.TEST.SPECIAL_NMS, cfg.TEST.TH, cfg.TEST.PRE_NMS_TOP_N, cfg.TEST.SELECT_CLASSES = "none", th, top_n, tuple(classes)
    return cfg


def _pack(rows_per_t, wh_orig, scale, flip, ranges, K):
    """rows_per_t[t][b] = list of (box in the ORIGINAL frame, score, label) -> dets (per transform rows sorted by score like the model's)."""
    dets = []
    for t, per_b in enumerate(rows_per_t):
        packed = np.zeros((len(wh_orig), K, 6), F)
        counts, wh = [], []
        for b, rows in enumerate(per_b):
            w, h = wh_orig[b]
            s = scale[t]
            ws, hs = int(w * s), int(h * s)
            assert len(rows) <= K
            if rows:
                bx = np.array([r[0] for r in rows], np.float64) * s
                if flip[t]:                                  # into the flipped frame: the merge flips it back
                    bx = np.stack([ws - bx[:, 2] - 1, bx[:, 1], ws - bx[:, 0] - 1, bx[:, 3]], 1)
                sc = np.array([r[1] for r in rows], F)
                o = np.argsort(-np.nan_to_num(sc, nan=2.0), kind="stable")
                packed[b, :len(rows)] = np.concatenate([bx[o], sc[o, None], np.array([r[2] for r in rows], np.float64)[o, None]], 1)
            counts.append(len(rows))
            wh.append((ws, hs))
        dets.append((torch.from_numpy(packed), counts, wh, flip[t], ranges[t]))
    return dets


def _rand_box(g, w, h, lo=4.0, hi=0.4):
    x1, y1 = g.uniform(0, 0.6 * w), g.uniform(0, 0.6 * h)
    return [x1, y1, x1 + g.uniform(lo, hi * w), y1 + g.uniform(lo, hi * h)]


CLASSES_MIXED = (5, 2, 9, 3, 7, 1)                          # out of order; 7 has no rows, 1 one row, 3 ROW_CAP rows, 9 ROW_CAP + 1; 6 and 11 outside


def draw_mixed(ranges_on=True, th=0.5, top_n=1000, seed=11):
    """B = 2, T = 4 (transforms 1 and 3 flipped, scales 1 / 1 / 1.5 / 0.75, transform 3 with a real area band when ranges_on).  Classes 1,
    3 and 9 sit in transform 0 (scale 1, no band that bites), so their counts are exact; one NaN score; labels 6 and 11 outside the list."""
    g = np.random.default_rng(seed)
    wh = [(96, 64), (50, 80)]
    pool = list(g.permutation(np.arange(1, 3000)).astype(F) / F(4096.0))
    rows_per_t = [[[] for _ in wh] for _ in range(4)]
    for b, (w, h) in enumerate(wh):
        for lab, n in ((1, 1), (3, ROW_CAP), (9, ROW_CAP + 1)):
            for _ in range(n):
                rows_per_t[0][b].append((_rand_box(g, w, h), pool.pop(), lab))
        for lab, n in ((5, 40), (2, 70), (6, 6), (11, 5)):
            for i in range(n):
                rows_per_t[1 + i % 3][b].append((_rand_box(g, w, h), pool.pop(), lab))
        r = rows_per_t[2][b][4]
        if b == 0:
            rows_per_t[2][b][4] = (r[0], F(np.nan), r[2])
    rng = ((0, 10000), (0, 10000), (0, 10000), (8, 30)) if ranges_on else (None,) * 4
    dets = _pack(rows_per_t, wh, (1.0, 1.0, 1.5, 0.75), (False, True, False, True), rng, 64)
    return dets, wh, make_cfg(CLASSES_MIXED, th, top_n)


def draw_one_class(seed=12, n=180, K=100):
    """Every row in ONE class (one workgroup per image does all the work; with ROW_CAP the workspace path, kept heads past the LDS list)."""
    g = np.random.default_rng(seed)
    wh = [(120, 90)]
    pool = list(g.permutation(np.arange(1, 1000)).astype(F) / F(1024.0))
    rows_per_t = [[[]], [[]]]
    for i in range(n):
        rows_per_t[i % 2][0].append((_rand_box(g, 120, 90, 3.0, 0.25), pool.pop(), 4))
    return _pack(rows_per_t, wh, (1.0, 2.0), (False, True), (None, None), K), wh, make_cfg((4,), 0.4, 1000)


def draw_all_suppressed(seed=13, n=40):
    """One class: the best row covers the image's object, every other row is that box jittered (IoU with it above 0.5): one survivor."""
    g = np.random.default_rng(seed)
    wh = [(80, 60)]
    rows = [([10.0, 10.0, 60.0, 50.0], F(0.99), 2)]
    for i in range(n - 1):
        j = g.uniform(-2.0, 2.0, 4)
        rows.append(([10.0 + j[0], 10.0 + j[1], 60.0 + j[2], 50.0 + j[3]], F((500 - i) / 1024.0), 2))
    return _pack([[rows]], wh, (1.0,), (False,), (None,), n), wh, make_cfg((2, 3), 0.5, 1000)


def draw_none_suppressed(seed=14):
    """Disjoint boxes on a grid, three classes, B = 3 (the third image has no rows at all): every row survives; top_n cuts with a tie kept."""
    g = np.random.default_rng(seed)
    wh = [(100, 100), (64, 64), (40, 40)]
    per_b = []
    for b, (w, h) in enumerate(wh[:2]):
        rows = []
        pool = list(g.permutation(np.arange(1, 200)).astype(F) / F(256.0))
        for i in range(36):
            cx, cy = (i % 6) * 0.16 * w + 1, (i // 6) * 0.16 * h + 1
            rows.append(([cx, cy, cx + 0.1 * w, cy + 0.1 * h], pool.pop(), (1, 2, 3)[i % 3]))
        per_b.append(rows)
    per_b.append([])
    return _pack([per_b], wh, (1.0,), (False,), (None,), 36), wh, make_cfg((3, 1, 2), 0.5, 1000)


def draw_equal_scores(seed=15):
    """Scores quantised to k / 8, so most rows tie: among overlapping rows of equal score the lower list position (the earlier transform,
    the earlier row) wins; two transforms carry the SAME rows, so every row has an exact duplicate of equal score later in the list."""
    g = np.random.default_rng(seed)
    wh = [(90, 70), (70, 90)]
    per_b = []
    for (w, h) in wh:
        per_b.append([(_rand_box(g, w, h, 6.0, 0.5), F(int(g.integers(1, 8)) / 8.0), int(g.integers(1, 4))) for _ in range(60)])
    return _pack([per_b, per_b, per_b], wh, (1.0, 1.0, 1.0), (False, False, True), (None,) * 3, 60), wh, make_cfg((1, 2, 3), 0.3, 25)


def toy_draws():
    """(name, dets, orig_wh, cfg) of every toy draw."""
    return [("mixed_ranges", *draw_mixed(True)), ("mixed_noranges_cut", *draw_mixed(False, top_n=30)), ("mixed_th0", *draw_mixed(True, th=0.0)),
            ("mixed_th_negative", *draw_mixed(True, th=-1.0, top_n=40)), ("one_class", *draw_one_class()),
            ("all_suppressed", *draw_all_suppressed()), ("none_suppressed", *draw_none_suppressed()), ("equal_scores", *draw_equal_scores())]


def large_dets(seed, T, B, K, live, wh_orig, n_cls, one_class_rows=0):
    """T x B x K slots with about `live` live rows per transform and image (N = T K rows go to the merge), distinct scores.  one_class_rows:
    that many rows of class 1 in transform 0 (K >= one_class_rows) -- a class above the LDS row cap."""
    g = np.random.default_rng(seed)
    pool = g.permutation(np.arange(1, T * B * K + 1)).astype(F) / F(1 << 20)
    dets = []
    for t in range(T):
        packed = np.zeros((B, K, 6), F)
        counts, wh = [], []
        for b, (w, h) in enumerate(wh_orig):
            s = (1.0, 1.5, 0.75, 2.0)[t % 4]
            ws, hs = int(w * s), int(h * s)
            n = one_class_rows if (t == 0 and one_class_rows) else int(g.integers(live - live // 8, live + live // 8 + 1))
            x1, y1 = g.uniform(0, 0.8 * ws, n), g.uniform(0, 0.8 * hs, n)
            rows = np.stack([x1, y1, x1 + g.uniform(2, 0.3 * ws, n), y1 + g.uniform(2, 0.3 * hs, n)], 1)
            sc = pool[(t * B + b) * K:(t * B + b) * K + n]
            lab = np.ones(n) if (t == 0 and one_class_rows) else g.integers(1, n_cls + 1, n)
            o = np.argsort(-sc, kind="stable")
            packed[b, :n] = np.concatenate([rows[o], sc[o, None], lab[o, None]], 1)
            counts.append(n)
            wh.append((ws, hs))
        dets.append((torch.from_numpy(packed), counts, wh, t % 2 == 1, None))
    return dets


def to_device(dets, device):
    return [(d[0].to(device),) + tuple(d[1:]) for d in dets]
