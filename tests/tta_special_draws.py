"""TEST INFRASTRUCTURE ONLY.  The random-shape sweep of the TEST.SPECIAL_NMS = 'soft-nms' / 'vote' / 'soft-vote' merges (mq_tta_merge_special,
mq_tta_merge_finalize_special, csrc/tta.hip), split into DRAWING and RUNNING like tests/fuzz_cases.py: the same draw runs through the emulation
of the kernel sources (tests/test_tta_special_sweep_cpu.py) and on the device (tests/test_gpu_tta_special_sweep.py), and a failing device
draw replays unchanged on the emulator.  tests/tta_special_cases.py holds ONE data set whose largest class has 64 rows and whose images
have 147 live rows: one wave and one 256-row chunk hold everything.  The draws here go past both.

A stream is made of ROUNDS of len(PLANS) draws per mode; draw k is plan k % len(PLANS) of round k // len(PLANS), seeded by (mode, seed, k)
alone, so it is the same case whatever the count, and `python tests/tta_special_draws.py <mode> <k>` regenerates it from nothing else.

A draw = dets for tta.merge (host tensors), orig_wh, the class list, mode, TEST.TH, TEST.PRE_NMS_TOP_N, row_cap, a `what` label, the
restated reference's answer (`want`, tests/tta_special_ref.py) and the number of (image, class) segments expected in the global workspace,
counted from the restated rows.  What a round varies (PLANS; test_the_draws_hold_what_they_claim reads it back from the restated rows):

  class sizes   live rows of one class in one image, each from SIZES = {0, 1, 2, 63, 64, 65, 255, 256, 257, 300, 513}: every round holds a
                class >= 257 (more than one 256-row trip of every `k += 256` loop, all four waves own rows), one in 65 .. 255, and classes of
                0, 1 and 2 rows.  The class list is out of order and holds a label without rows; some rows carry labels outside the list
                (one below and one above the list's largest label); every image has one NaN score.
  live rows     per image at or next to a multiple of 256 (255, 256, 257, 768, 769, 1024, 1025: the tiles of tta_cut_rank_kernel /
                tta_rank_final_kernel and the trips of the staging loop) wherever the sizes allow it -- 300 = 256 + 44, and no handful of the
                other sizes brings that to 0 or +-1 modulo 256, so the images of the plans with a 300-row class fall where they fall (624,
                880, 814 rows: still 3 and 4 tiles).  B = 1 .. 3 with ragged row counts, one image of plan 2 has no live row at all.
  transforms    T = 1 .. 3, scales and flips drawn, one transform with an area band (tiny decoy rows die in it), ragged counts; K is the
                largest count, so one transform is full.  T = 1 carries no band (the kernel's band == NULL path).
  row_cap       None (1024: all in LDS) / 32 / 256: workspace counts 0, 1 and > 1 in every round, a 257-row class behind 768 rows of earlier
                classes in the workspace (plan 2), a 256-row class that just stays in LDS beside a 257-row one that does not (plan 4).
  top_n         no cut, the expected output count (`total > top_n` against `>=`), count - 1, 1, a middle value; counts come from the
                restated reference, never from the product.  vote / soft-vote, plan 5: one score repeated in two DIFFERENT classes exactly
                at the cut (kthvalue keeps both, and so does `>= thr`); scores stay distinct inside a class.
  boxes         vote / soft-vote: 'r' random boxes, half of them jittered around m / 10 anchors so that clusters of many members form (their
                members are spread over the whole score order: every wave contributes to a voted sum); 'o' one cluster of the whole class;
                'a' a grid with gaps, no overlaps.  soft-nms: clusters of <= 8 jittered boxes, one cluster per cell of a grid whose cells are
                4 px and more apart: the IoU between cells is exactly 0 and the factor exp(-0) exactly 1, so a row's effective decays stay
                below 8 and the restated reference's own margins hold (uniformly random boxes at these sizes fail them nearly always).
  scores        distinct multiples of 2^-14.

ACCEPTANCE (tta_special_ref's per-row margins): a soft-nms draw whose reference shows thr_ratio, pick_ratio or cut_ratio < 2 is not run, nor
is a draw of any mode with a repeated score inside a class, on input or output.  At most MAX_REJECTED = 10 % of the drawn cases of a mode
may be rejected; both suites assert it from STATS, the counts kept while drawing.
Measured with this drawing code, numpy only, 25 rounds (200 draws) per mode at seed 0: see MEASURED below.

The comparison is tta_special_cases.compare, unchanged.  `run` adds what the contract of ops.tta_merge states beside it: the workspace
count, finite outputs, and rows past counts[b] of the three output arrays left as they were allocated.

Replay:  python tests/tta_special_draws.py <mode> <draw> [--seed S] [--device cpu|cuda] [--halo]
         (--device cpu: through the emulation, every argument against a guard page; --halo: between NaN poison halos, tests/halo.py)"""
import contextlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import tta_special_cases as sc  # noqa: E402
import tta_special_ref as ref  # noqa: E402

# rejected / drawn per mode, 25 rounds at seed 0 (numpy only), and the smallest ratio among the accepted soft-nms draws
MEASURED = {"soft-nms": "5 of 200 rejected (draws 44, 54, 93, 181, 191: pick_ratio 0.62 .. 1.70; smallest accepted ratio 2.09)", "vote": "0 of 200 rejected",
            "soft-vote": "0 of 200 rejected"}

SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 300, 513)
MODE_SEED = {"soft-nms": 7101, "vote": 7202, "soft-vote": 7303}
TH = {"soft-nms": (0.3, 0.2), "vote": (0.5, 0.45), "soft-vote": (0.5, 0.45)}      # soft-nms: on the score; votes: on the IoU
INFERENCE_TH = 0.05
DEFAULT_CAP = 1024                                          # ops.TTA_SPECIAL_ROW_CAP (asserted in run)
NO_CUT = 100000
MAX_REJECTED = 0.10
MIN_RATIO = 2.0
SCALES = (1.0, 1.5, 0.75, 1.25)
BAND = (8, 48)                                              # the banded transform keeps boxes of 64 .. 2304 px^2 (its own frame)
STATS = {}                                                  # mode -> {"drawn", "rejected"} of everything drawn so far

# sizes per image in class-list position order, vote kinds per position ('r' random, 'o' one cluster, 'a' apart), row_cap, cut
PLANS = (
    dict(T=2, sizes=[(300, 257, 64, 1, 2, 0)], kinds="rroooo", cap=None, cut="none"),                                   # 624
    dict(T=3, sizes=[(513, 65, 64, 63, 63, 1, 0), (255, 2, 0, 0, 0, 0, 0)], kinds="roarroo", cap=256, cut="count"),     # 769, 257
    dict(T=3, sizes=[(255, 513, 257, 0), (0, 0, 0, 0), (256, 1, 0, 0)], kinds="rrro", cap=256, cut="count-1"),          # 1025, 0, 257
    dict(T=1, sizes=[(63, 64, 65, 63, 0, 1)], kinds="oarroo", cap=32, cut="one"),                                       # 256
    dict(T=2, sizes=[(256, 255, 257, 0), (2, 255, 0, 0)], kinds="oaro", cap=256, cut="middle"),                         # 768, 257
    dict(T=3, sizes=[(1, 513, 255, 0, 255)], kinds="orror", cap=None, cut="tie"),                                       # 1024
    dict(T=2, sizes=[(300, 513, 65, 2, 0), (513, 300, 1, 0, 0)], kinds="rrroo", cap=32, cut="count"),                   # 880, 814
    dict(T=None, sizes=None, kinds=None, cap="any", cut="any"),                                                         # everything drawn
)
CUTS = ("none", "count", "count-1", "one", "middle")


# ------------------------------------------------------------------------------------------------------------------ boxes
def _clustered(g, m, w, h):
    """clusters of <= 8 jittered boxes, one per cell of a 40 px grid; boxes of different cells are >= 4 px apart (the +1 of the IoU reaches 1 px)"""
    pitch = 40
    nx, ny = int(w) // pitch, int(h) // pitch
    while True:
        sizes, left = [], m
        while left > 0:
            s = int(min(left, g.integers(1 if m <= 300 else 3, 9)))
            sizes.append(s)
            left -= s
        if len(sizes) <= nx * ny:
            break
    cells = g.permutation(nx * ny)[:len(sizes)]
    out = []
    for c, s in zip(cells, sizes):
        ox, oy = (c % nx) * pitch, (c // nx) * pitch
        bw, bh = g.uniform(18, 26, 2)
        amp = g.uniform(1, 5)                                  # per cluster: IoUs from about 0.4 to 0.9, one to several decays survive
        for _ in range(s):
            j = g.uniform(-amp, amp, 4)
            out.append([ox + 4 + j[0], oy + 4 + j[1], ox + 4 + bw + j[2], oy + 4 + bh + j[3]])      # inside [ox - 1, ox + 35]
    return out


def _random(g, m, w, h):
    """half the rows jittered around m / 10 anchors (clusters of many members at IoU >= 0.45), half uniformly random"""
    na = max(1, m // 10)
    ax, ay = g.uniform(0, 0.7 * w, na), g.uniform(0, 0.7 * h, na)
    aw, ah = g.uniform(20, 0.3 * w, na), g.uniform(20, 0.3 * h, na)
    out = []
    for i in range(m):
        if i % 2 == 0:
            a = int(g.integers(na))
            j = g.uniform(-0.08, 0.08, 4) * [aw[a], ah[a], aw[a], ah[a]]
            out.append([ax[a] + j[0], ay[a] + j[1], ax[a] + aw[a] + j[2], ay[a] + ah[a] + j[3]])
        else:
            x, y = g.uniform(0, 0.7 * w), g.uniform(0, 0.7 * h)
            out.append([x, y, x + g.uniform(8, 0.3 * w), y + g.uniform(8, 0.3 * h)])
    return out


def _one_cluster(g, m, w, h):
    bw, bh = g.uniform(24, 40, 2)
    x, y = g.uniform(0, w - 50), g.uniform(0, h - 50)
    return [list(np.array([x, y, x + bw, y + bh]) + g.uniform(-0.6, 0.6, 4)) for _ in range(m)]


def _apart(g, m, w, h):
    pitch = 20
    nx, ny = int(w) // pitch, int(h) // pitch
    assert m <= nx * ny
    return [[(c % nx) * pitch + 2, (c // nx) * pitch + 2, (c % nx) * pitch + 2 + g.uniform(8, 12), (c // nx) * pitch + 2 + g.uniform(8, 12)]
            for c in g.permutation(nx * ny)[:m]]


def _class_boxes(g, mode, kind, m, w, h):
    if m == 0:
        return []
    if mode == "soft-nms":
        return _clustered(g, m, w, h)
    return {"r": _random, "o": _one_cluster, "a": _apart}[kind](g, m, w, h)


# ------------------------------------------------------------------------------------------------------------------ drawing
def _draw_plan(g, plan):
    """the drawn plan (index 7): B, T, 3 .. 6 classes per image from SIZES, at most one of 300 / 513 per image"""
    if plan["sizes"] is not None:
        return plan
    B, L = int(g.integers(1, 4)), int(g.integers(4, 7))
    sizes = []
    for _ in range(B):
        row = [int(g.choice(SIZES[:9])) for _ in range(L)]
        if g.random() < 0.5:
            row[int(g.integers(L))] = int(g.choice(SIZES[9:]))
        sizes.append(tuple(row))
    sizes[0] = (int(g.choice(SIZES[3:9])),) + sizes[0][1:]                     # the image the cut is placed on has rows
    z = int(g.integers(1, L))                                                  # a label of the list without rows
    sizes = [r[:z] + (0,) + r[z + 1:] for r in sizes]
    return dict(T=int(g.integers(1, 4)), sizes=sizes, kinds="".join(g.choice(list("rrroa"), L)), cap=[None, 32, 256][int(g.integers(3))],
                cut=CUTS[int(g.integers(len(CUTS)))])


def _pack(g, mode, plan, classes, outside, wh, pool):
    """rows of every image in its original frame, dealt to the transforms -> dets for tta.merge"""
    T, B = plan["T"], len(wh)
    scale = [SCALES[0]] + [float(s) for s in g.choice(SCALES[1:], T - 1, replace=False)]
    flip = [bool(g.integers(2)) for _ in range(T)]
    tb = int(g.integers(1, T)) if T > 1 else -1                                # the banded transform (never the first)
    per, used = [], 0
    for b, (w, h) in enumerate(wh):
        rows = []                                                              # (box, label, fixed transform or None)
        for pos, m in enumerate(plan["sizes"][b]):
            kind = plan["kinds"][pos] if m > 2 else "o"                        # a class of two rows: an overlapping pair
            rows += [(bx, classes[pos], None) for bx in _class_boxes(g, mode, kind, m, w, h)]
        for lab in outside:
            for _ in range(int(g.integers(2, 6))):
                x, y = g.uniform(0, 0.6 * w), g.uniform(0, 0.6 * h)
                rows.append(([x, y, x + g.uniform(8, 0.3 * w), y + g.uniform(8, 0.3 * h)], lab, 0))
        if tb >= 0:                                                            # decoys: in the list, too small for the band
            for _ in range(3):
                x, y = g.uniform(0, 0.8 * w), g.uniform(0, 0.8 * h)
                rows.append(([x, y, x + 2, y + 2], classes[0], tb))
        nan_row = len(rows)
        rows.append(([0.2 * w, 0.2 * h, 0.5 * w, 0.5 * h], classes[int(g.integers(len(classes)))], 0))
        # deal: free rows to random transforms (ragged shares), into the band only when the area is well inside it
        share = g.dirichlet(np.full(T, 3.0))
        where = np.zeros(len(rows), np.int64)
        for i, (bx, _, fixed) in enumerate(rows):
            if fixed is not None:
                where[i] = fixed
                continue
            t = int(g.choice(T, p=share))
            if t == tb:
                s = scale[tb]
                a = ((bx[2] - bx[0]) * s + 1) * ((bx[3] - bx[1]) * s + 1)
                if not BAND[0] ** 2 * 1.1 < a < BAND[1] ** 2 * 0.9:
                    t = 0
            where[i] = t
        sco = pool[used:used + len(rows)].copy()
        used += len(rows)
        sco[nan_row] = np.nan
        per.append((rows, where, sco))
    K = max(1, max(int((where == t).sum()) for _, where, _ in per for t in range(T)))
    dets = []
    for t in range(T):
        packed, counts, whs = np.zeros((B, K, 6), np.float32), [], []
        for b, (w, h) in enumerate(wh):
            rows, where, sco = per[b]
            part = np.nonzero(where == t)[0]
            s = scale[t]
            ws, hs = int(w * s), int(h * s)
            whs.append((ws, hs))
            counts.append(len(part))
            if not len(part):
                continue
            bx = np.array([rows[i][0] for i in part], np.float64) * s
            if flip[t]:                                                        # into the flipped frame: the merge flips it back
                bx = np.stack([ws - bx[:, 2] - 1, bx[:, 1], ws - bx[:, 0] - 1, bx[:, 3]], 1)
            o = np.argsort(-np.nan_to_num(sco[part], nan=2.0), kind="stable")  # score-sorted like the model's rows
            lab = np.array([rows[i][1] for i in part], np.float64)
            packed[b, :len(part)] = np.concatenate([bx[o], sco[part][o, None], lab[o, None]], 1)
        rng = None if T == 1 else (BAND if t == tb else (0, 10000))
        dets.append((torch.from_numpy(packed), counts, whs, flip[t], rng))
    return dets, dict(scale=scale, flip=flip, band=tb)


def _accept(mode, want):
    for w in want:
        m = w["margins"]
        if not (m["in_distinct"] and m["out_distinct"]):
            return "a score repeats inside a class"
        if mode == "soft-nms":
            for key in ("thr_ratio", "pick_ratio", "cut_ratio"):
                if m[key] < MIN_RATIO:
                    return f"{key} {m[key]:.2f} < {MIN_RATIO}"
    return None


def _tie_at_the_cut(dets, b, cols, rows_b):
    """two output rows of DIFFERENT classes, neighbours in the score order of image b's un-cut output: the lower one's input score is
    raised to the higher one's (no output score lies between them, and every head that absorbed a row between them scores higher than
    both: the clusters stay as they are) -> top_n with the cut between the two, or None"""
    s, lab = cols[1], cols[2]
    order = np.argsort(-s, kind="stable")
    n = len(order)
    in_s = rows_b[1]
    for p in range(n // 3, n - 2):
        a, c = order[p], order[p + 1]
        if lab[a] != lab[c] and s[a] > s[c] and (in_s == s[c]).sum() == 1 and (in_s == s[a]).sum() == 1:
            for packed, counts, *_ in dets:
                hit = (packed[b, :counts[b], 4] == float(s[c])).nonzero()
                if len(hit):
                    packed[b, int(hit[0]), 4] = float(s[a])
                    return p + 1
    return None


def draw(mode, k, seed=0):
    """draw k of `mode` (module docstring)"""
    plan_i = k % len(PLANS)
    g = np.random.default_rng([MODE_SEED[mode], seed, k])
    plan = _draw_plan(g, PLANS[plan_i])
    L = len(plan["sizes"][0])
    labels = g.permutation(np.arange(1, 24))
    classes = tuple(int(c) for c in labels[:L])
    if list(classes) == sorted(classes):                                       # out of order, whatever was drawn
        classes = classes[::-1]
    below = [int(c) for c in labels[L:] if c < max(classes)]
    outside = (below[0] if below else int(labels[L]), 24 + int(g.integers(8)))  # inside cls_rank without a rank / past its end
    wh = [(int(g.integers(600, 721)), int(g.integers(440, 521))) for _ in plan["sizes"]]
    pool = g.permutation(np.arange(1, 16384)).astype(np.float32) / np.float32(16384.0)
    th = TH[mode][int(g.integers(2))]
    dets, tinfo = _pack(g, mode, plan, classes, outside, wh, pool)
    rows = sc.prep_restated(dets, wh)
    cols = [ref.merge_classes(bx, s, lb, classes, mode, th, INFERENCE_TH) for bx, s, lb in rows]
    live = [b for b, s in enumerate(plan["sizes"]) if sum(s)]
    b0 = live[0]
    count = len(cols[b0][0][1])
    cut = plan["cut"]
    if cut == "tie" and mode == "soft-nms":
        cut = "middle"                                                         # decayed scores cannot be made to tie: a middle cut
    if cut == "tie":
        top_n = _tie_at_the_cut(dets, b0, cols[b0][0], rows[b0])
        assert top_n is not None, "no two neighbouring output rows of different classes"
        rows = sc.prep_restated(dets, wh)
        cols[b0] = ref.merge_classes(*rows[b0], classes, mode, th, INFERENCE_TH)
    else:
        top_n = {"none": NO_CUT, "count": count, "count-1": count - 1, "one": 1, "middle": int(g.integers(count // 4, 3 * count // 4 + 1))}[cut]
    want = [ref.cut_top_n(c, m, top_n) for c, m in cols]
    cap = plan["cap"]
    eff_cap = DEFAULT_CAP if cap is None else cap
    nws = 0
    for bx, s, lb in rows:                                                     # segments past the cap, from the restated rows
        ok = ~np.isnan(s)
        nws += sum(int((lb[ok] == c).sum()) > eff_cap for c in classes)
    st = STATS.setdefault(mode, {"drawn": 0, "rejected": 0})
    why = _accept(mode, want)
    st["drawn"] += 1
    st["rejected"] += why is not None
    what = (f"{mode} draw {k} (plan {plan_i}): B {len(wh)} T {plan['T']} sizes {plan['sizes']} th {th} cut {cut} top_n {top_n} cap {cap} "
            f"flip {tinfo['flip']} band {tinfo['band']}")
    return dict(mode=mode, k=k, plan=plan_i, dets=dets, orig_wh=wh, classes=classes, th=th, top_n=top_n, row_cap=cap, what=what, want=want,
                rows=rows, sizes=plan["sizes"], kinds=plan["kinds"], cut=cut, cut_image=b0, uncut_count=count, workspace_classes=nws,
                rejected=why, T=plan["T"])


def cases(mode, rounds=1, seed=0):
    """draws 0 .. rounds * len(PLANS) - 1 of `mode`; a rejected draw is yielded too (c["rejected"] says why) so that k keeps its meaning"""
    for k in range(rounds * len(PLANS)):
        yield draw(mode, k, seed)


def check_rejections(mode):
    st = STATS[mode]
    assert st["rejected"] <= MAX_REJECTED * st["drawn"], f"{mode}: the reference's own margins rejected {st}"


# ------------------------------------------------------------------------------------------------------------------ running
def make_cfg(case):
    from mq_det_amd import get_cfg
    cfg = get_cfg()
    cfg.TEST.SPECIAL_NMS, cfg.TEST.TH, cfg.TEST.PRE_NMS_TOP_N, cfg.TEST.SELECT_CLASSES = case["mode"], case["th"], case["top_n"], case["classes"]
    cfg.MODEL.RETINANET.INFERENCE_TH = INFERENCE_TH
    return cfg


_FILL = {torch.float32: -12345.0, torch.int64: -777, torch.int32: -777, torch.uint8: 0xA5}


class _FilledTorch:
    """`torch` as mq_det_amd.ops sees it while a draw runs: empty() hands out memory that holds a known value, so that a row the merge
    did not write can be told from one it did"""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def empty(*shape, dtype=None, device=None):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        return torch.full(shape, _FILL[dtype], dtype=dtype, device=device) if dtype in _FILL else torch.empty(shape, dtype=dtype, device=device)


@contextlib.contextmanager
def watched_outputs():
    """inside: ops.tta_merge allocates filled memory and its return values are kept -> list of (boxes, scores, labels, counts, dropped)"""
    from mq_det_amd import ops
    seen, real_torch, real_merge = [], ops.torch, ops.tta_merge

    def spy(*a, **kw):
        out = real_merge(*a, **kw)
        seen.append(out)
        return out
    ops.torch, ops.tta_merge = _FilledTorch(), spy
    try:
        yield seen
    finally:
        ops.torch, ops.tta_merge = real_torch, real_merge


def run(case, device):
    """the product on the draw (the library mq_det_amd.ops holds: the device's, or the emulation's on CPU tensors) against case["want"]"""
    from mq_det_amd import ops, tta
    assert case["rejected"] is None, case["rejected"]
    assert ops.TTA_SPECIAL_ROW_CAP == DEFAULT_CAP
    tta._WARNED_CLASSES = True
    stats = {}
    with watched_outputs() as seen:
        got = tta.merge(sc.to_device(case["dets"], device), case["orig_wh"], make_cfg(case), device, row_cap=case["row_cap"], stats=stats)
        if device.type == "cuda":
            torch.cuda.synchronize()
    what = case["what"]
    assert stats["workspace_classes"] == case["workspace_classes"], (what, stats, case["workspace_classes"])
    got = sc.host(got)
    for r, wh in zip(got, case["orig_wh"]):
        assert r.size == wh and r.mode == "xyxy" and r.fields() == ["scores", "labels"], what
        assert torch.isfinite(r.bbox).all() and torch.isfinite(r.get_field("scores")).all(), what
    sc.compare(case["mode"], case["th"], got, case["want"], what)
    # rows past counts[b]: not written (ops.tta_merge: "rows past counts[b] are junk", i.e. whatever the allocation held)
    (boxes, scores, labels, n_out, _), = seen
    n_out = n_out.tolist()
    assert n_out == [len(w["scores"]) for w in case["want"]], what
    for b, n in enumerate(n_out):
        for name, t in (("boxes", boxes), ("scores", scores), ("labels", labels)):
            tail = t[b, n:].cpu()
            assert bool((tail == _FILL[t.dtype]).all()), f"{what}: image {b}: {name} written past its {n} rows"


# ------------------------------------------------------------------------------------------------------------------ ties across waves
TIE_GROUPS = ((60, 68), (120, 136), (188, 196), (250, 263))       # staged slots that share a score: across 63|64, 127|128, 191|192 and 255|256
TIE_ORDERS = ("ascending", "reversed", "shuffled")


def tie_case(order):
    """One class of 300 mutually disjoint rows.  Rows of equal score are NEIGHBOURS in the staged (score) order, so no two of them can sit
    at far-apart slots; the groups are laid across the boundaries between the four waves (slots 63|64, 127|128, 191|192) and across the
    256-row trip (255|256, where thread 0 of wave 0 meets thread 255 of wave 3), one of them 16 rows long.  `order`: how the rows are
    packed, i.e. which ORIGINAL ROW every box has.  -> (dets, orig_wh, classes, packed rows in the order the rule of csrc/tta.hip gives:
    score descending, original row ascending).  The reference leaves the order of equal scores to numpy's unstable argsort."""
    m, wh = 300, (400, 300)
    score = (16000.0 - 8.0 * np.arange(m)) / 16384.0
    for lo, hi in TIE_GROUPS:
        score[lo:hi] = score[lo]
    i = np.arange(m)
    box = np.stack([(i % 20) * 16 + 2, (i // 20) * 16 + 2, (i % 20) * 16 + 12, (i // 20) * 16 + 12], 1).astype(np.float64)
    rows = np.concatenate([box, score[:, None], np.full((m, 1), 3.0)], 1).astype(np.float32)
    perm = {"ascending": i, "reversed": i[::-1], "shuffled": np.random.default_rng(11).permutation(m)}[order]
    packed = rows[perm]
    want = packed[np.lexsort((np.arange(m), -packed[:, 4].astype(np.float64)))]
    return [(torch.from_numpy(packed[None].copy()), [m], [wh], False, None)], [wh], (5, 3), want


def run_ties(mode, device):
    """every packing order, without a cut and with the cut inside the first group of equal scores (kthvalue keeps the whole group)"""
    from mq_det_amd import tta
    for order in TIE_ORDERS:
        dets, wh, classes, want = tie_case(order)
        for top_n, kept in ((NO_CUT, 300), (64, TIE_GROUPS[0][1])):
            case = dict(mode=mode, th=TH[mode][0], top_n=top_n, classes=classes)
            for cap in (None, 256):
                got = sc.host(tta.merge(sc.to_device(dets, device), wh, make_cfg(case), device, row_cap=cap))[0]
                what = f"ties {mode} {order} top_n {top_n} cap {cap}"
                assert len(got) == kept, (what, len(got))
                assert np.array_equal(got.get_field("scores").numpy(), want[:kept, 4]), what
                assert np.array_equal(got.bbox.numpy(), want[:kept, :4]), what
                assert (got.get_field("labels").numpy() == 3).all(), what


def run_cut_contract(device):
    """mq_tta_merge_finalize_special alone on rows of its own, n = 600 and 257 of N = 700 slots (three tiles, three workgroups per image):
    thr [B] is the top_n-th largest kept score when MORE than top_n rows are kept and -inf otherwise ("-inf: no cut", csrc/tta.hip), and
    the output is the kept rows at or above it in seq order."""
    from mq_det_amd import ops
    lib = ops.load_library()
    g = np.random.default_rng(23)
    B, N, nv = 2, 700, [600, 257]
    scores = g.permutation(np.arange(1, 16384))[:B * N].reshape(B, N).astype(np.float32) / np.float32(16384.0)
    keep = (g.random((B, N)) < 0.7).astype(np.uint8)
    seq = np.stack([g.permutation(N) for _ in range(B)]).astype(np.int32)
    boxes = g.uniform(0, 100, (B, N, 4)).astype(np.float32)
    total = [int(keep[b, :nv[b]].sum()) for b in range(B)]
    put = lambda a: torch.from_numpy(a).to(device)      # noqa: E731
    t_scores, t_keep, t_seq, t_boxes = put(scores), put(keep), put(seq), put(boxes)
    labels_s, cls_rank, nvalid = torch.ones(B, N, dtype=torch.int32, device=device), put(np.array([-1, 0], np.int32)), put(np.array(nv, np.int32))
    for top_n in (0, 1, total[1] - 1, total[1], total[1] + 1, total[0] - 1, total[0], total[0] + 1):
        thr = torch.full((B,), 7.0, dtype=torch.float32, device=device)
        boxes_o = torch.full((B, N, 4), -1.0, dtype=torch.float32, device=device)
        scores_o = torch.full((B, N), -1.0, dtype=torch.float32, device=device)
        labels_o, counts = torch.full((B, N), -1, dtype=torch.int64, device=device), torch.zeros(B, dtype=torch.int32, device=device)
        ops._chk(lib.mq_tta_merge_finalize_special(ops._ptr(t_boxes), ops._ptr(t_scores), ops._ptr(labels_s), ops._ptr(t_seq), ops._ptr(t_keep),
                                                   ops._ptr(nvalid), ops._ptr(thr), ops._ptr(cls_rank), ops._ptr(boxes_o), ops._ptr(scores_o),
                                                   ops._ptr(labels_o), ops._ptr(counts), B, N, top_n, ops._stream()), "mq_tta_merge_finalize_special")
        thr, counts, scores_o, boxes_o = thr.cpu().numpy(), counts.cpu().numpy(), scores_o.cpu().numpy(), boxes_o.cpu().numpy()
        for b in range(B):
            idx = np.nonzero(keep[b, :nv[b]])[0]
            kept = np.sort(scores[b, idx])[::-1]
            want_thr = kept[top_n - 1] if total[b] > top_n > 0 else -np.inf
            assert thr[b] == want_thr, (top_n, b, thr[b], want_thr, total[b])
            out = idx[scores[b, idx] >= want_thr]
            out = out[np.argsort(seq[b, out])]
            assert counts[b] == len(out), (top_n, b)
            assert np.array_equal(scores_o[b, :len(out)], scores[b, out]) and np.array_equal(boxes_o[b, :len(out)], boxes[b, out]), (top_n, b)
            assert (scores_o[b, len(out):] == -1.0).all(), (top_n, b)


def replay_line(mode, k, seed=0, device="cpu", halo=False):
    return f"python tests/tta_special_draws.py {mode} {k}" + (f" --seed {seed}" if seed else "") + f" --device {device}" + (" --halo" if halo else "")


def _main(argv):
    import argparse
    ap = argparse.ArgumentParser(description="regenerate draw k of a mode and run it alone")
    ap.add_argument("mode", choices=ref.MODES)
    ap.add_argument("draw", type=int)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", choices=("cpu", "cuda"), default="cpu")
    ap.add_argument("--halo", action="store_true")
    a = ap.parse_args(argv)
    case = draw(a.mode, a.draw, a.seed)
    print(case["what"], flush=True)
    if case["rejected"]:
        print("  not run: " + case["rejected"])
        return 0
    with contextlib.ExitStack() as st:
        if a.device == "cuda":
            from mq_det_amd import ops
            ops.load_library()
            ops.configure()
            dev = torch.device("cuda:0")
        else:
            import simt
            from simt import guard
            st.enter_context(simt.installed())
            if not a.halo:
                st.enter_context(guard.pointer_guard())
            dev = torch.device("cpu")
        if a.halo:
            from halo import poisoned_args
            st.enter_context(poisoned_args("nan"))
        run(case, dev)
    print("draw ok")
    return 0


if __name__ == "__main__":
    sys.exit(_main(sys.argv[1:]))
