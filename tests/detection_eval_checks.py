"""Shared checks of the detection evaluation loop (mq_det_amd.detection, csrc/eval_rows.hip, the evaluators' `update_packed`), run by
tests/test_detection_eval_cpu.py on CPU tensors through the kernel-source emulation and by tests/test_gpu_detection_eval.py on the device.

The rows the kernel must give are STATED here in numpy fp32, without the code under test: for the LVIS evaluator the four lines of the
engine's `resize_box` (a multiply by the fp32 ratio) and `convert_to_xywh`; for the COCO evaluator tests/coco_eval_ref.result_rows (pinned to
the reference by tests/golden/coco_eval_prepare) for the rows of known labels, and the same arithmetic with the legacy + 1 for the rest.
Every comparison of rows is on the bits; NaN categories compare as NaN-in-the-same-place."""
import json
import math
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import coco_eval_ref  # noqa: E402
from mq_det_amd.config import get_cfg  # noqa: E402
from mq_det_amd.detection import TIE_OVERFLOW_WARNING, evaluate_detection  # noqa: E402
from mq_det_amd.evaluation import CocoAPEvaluator, FixedAPAccumulator, LvisFixedAPEvaluator, _ResultRows  # noqa: E402
from mq_det_amd.modeling.detector import GeneralizedVLRCNN_New  # noqa: E402

FILL = -7.0                                     # what the row buffers hold before a launch: untouched rows still hold it


# ---------------------------------------------------------------------------------------------- the statement
class Image:
    """one image of an entry table: id, network input size and target size as (width, height)"""

    def __init__(self, image_id, in_size, out_size):
        self.id, self.in_size, self.out_size = image_id, in_size, out_size
        self.rw, self.rh = float(out_size[0]) / float(in_size[0]), float(out_size[1]) / float(in_size[1])


def live_count(raw, K2, candidate):
    raw = int(raw)
    n = raw if candidate else raw & 0xFFFF
    return max(0, min(n, K2)), 0 if candidate else (raw >> 16) & 1


def statement(packed, counts, blocks, mode, candidate=False, label_map=None):
    """packed [items, K2, 6] fp32 / counts [items] numpy, blocks = [(Image, [items of the image in output order])] -> (rows fp32 [n, 7 | 8],
    overflow bit).  mode "lvis": resize_box + convert_to_xywh, the label as category, 7 columns.  mode "coco": BoxList.resize +
    convert("xywh") (+ 1), labels through label_map (NaN where it lacks one), 8 columns with the mark on the first row of an image's
    block, a placeholder row for an image without a detection."""
    K2 = packed.shape[1]
    out, over = [], 0
    for img, items in blocks:
        live = []
        for it in items:
            n, o = live_count(counts[it], K2, candidate)
            over |= o
            live.append(packed[it, :n])
        d = np.concatenate(live).astype(np.float32).reshape(-1, 6)
        ratio = np.array([img.rw, img.rh, img.rw, img.rh]).astype(np.float32)
        b = d[:, :4] * ratio                                                   # BoxList.resize: fp32 boxes times the ratio as fp32
        assert b.dtype == np.float32
        ids = np.full(len(d), img.id, np.float32)
        if mode == "lvis":                                                     # convert_to_xywh: (xmin, ymin, xmax - xmin, ymax - ymin)
            out.append(np.stack([ids, d[:, 5], d[:, 4], b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1))
            continue
        one = np.float32(1)
        cat = np.array([label_map.get(int(l), math.nan) for l in d[:, 5]], np.float32).reshape(-1)
        mark = np.zeros(len(d), np.float32)
        mark[:1] = 1
        rows = np.stack([ids, cat, d[:, 4], b[:, 0], b[:, 1], b[:, 2] - b[:, 0] + one, b[:, 3] - b[:, 1] + one, mark], 1)
        if len(d) == 0:
            rows = np.array([[img.id, math.nan, 0, 0, 0, 0, 0, 1]], np.float32)
        else:                                                                  # the rows of known labels = the restated prepare_for_coco_detection
            gt = {"images": [{"id": img.id, "width": img.out_size[0], "height": img.out_size[1]}], "categories": []}
            want = coco_eval_ref.result_rows([(img.id, img.in_size, d[:, :4], d[:, 4], d[:, 5].astype(np.int64))], gt, label_map)
            assert np.array_equal(rows[~np.isnan(cat)][:, :7].astype(np.float64), want)
        out.append(rows)
    cols = 7 if mode == "lvis" else 8
    rows = np.concatenate(out).astype(np.float32).reshape(-1, cols) if out else np.zeros((0, cols), np.float32)
    return rows, over


def same_rows(got, want):
    """bit equality; a NaN category equals a NaN category"""
    got = torch.as_tensor(got).detach().cpu().contiguous().clone()
    want = torch.as_tensor(want).detach().cpu().contiguous().clone()
    assert got.dtype == want.dtype == torch.float32 and got.shape == want.shape, (got.shape, want.shape)
    gn, wn = torch.isnan(got[:, 1]), torch.isnan(want[:, 1])
    assert torch.equal(gn, wn), "NaN categories in other places"
    got[gn, 1] = 0
    want[wn, 1] = 0
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (got.view(torch.int32) != want.view(torch.int32)).nonzero()[:8]


def image_major(images, g):
    """2 images x g chunks: the blocks in image-major order out of the forward's chunk-major items"""
    B = len(images)
    return [(img, [c * B + b for c in range(g)]) for b, img in enumerate(images)]


def launch(ops, device, packed, counts, blocks, mode, candidate=False, label_map=None, tail=64, exact=False):
    """the kernel through ops.eval_rows on `device` -> (rows written, the whole buffer, capacity, state).  The buffer is `tail` rows longer than the
    capacity and filled with FILL; exact: a buffer of the capacity alone, in storage of its own (for the guard pages / halos)."""
    items, K2 = packed.shape[:2]
    ent = [(it, img, n == 0) for img, its in blocks for n, it in enumerate(its)]
    table = ops.eval_rows_table([e[0] for e in ent], [float(e[1].id) for e in ent], [e[1].rw for e in ent], [e[1].rh for e in ent],
                                [e[2] for e in ent], items, device)
    cols = 7 if mode == "lvis" else 8
    cap = len(ent) * K2 + (len(blocks) if mode == "coco" else 0)
    buf = torch.full((cap + (0 if exact else tail), cols), FILL, dtype=torch.float32, device=device)
    state = torch.full((2,), -5, dtype=torch.int32, device=device)
    kw = {}
    if mode == "coco":
        keys = sorted(label_map)
        kw = dict(plus_one=True, placeholder=True, lbl_keys=torch.tensor(keys, dtype=torch.int32, device=device),
                  lbl_vals=torch.tensor([float(label_map[k]) for k in keys], dtype=torch.float32, device=device))
    ops.eval_rows(torch.from_numpy(packed).to(device), torch.from_numpy(counts.astype(np.int32)).to(device), table, buf[:cap], state, cols=cols,
                  candidate=candidate, **kw)
    n, over = state.cpu().tolist()
    return buf[:n].cpu(), buf.cpu(), cap, (n, over)


def check(ops, device, packed, counts, blocks, mode, candidate=False, label_map=None, exact=False):
    want, over = statement(packed, counts, blocks, mode, candidate, label_map)
    got, buf, cap, (n, got_over) = launch(ops, device, packed, counts, blocks, mode, candidate, label_map, exact=exact)
    assert n == len(want) <= cap and got_over == over, (n, len(want), got_over, over)
    same_rows(got, want)
    assert torch.equal(buf[n:], torch.full_like(buf[n:], FILL)), "rows behind the last one were written"
    return want


def random_packed(rng, items, K2, labels=(1, 2, 3, 4, 5, 6), span=1000.0):
    p = np.zeros((items, K2, 6), np.float32)
    x1, y1 = rng.random((items, K2)) * span, rng.random((items, K2)) * span
    p[..., 0], p[..., 1] = x1, y1
    p[..., 2], p[..., 3] = x1 + rng.random((items, K2)) * span * 0.5, y1 + rng.random((items, K2)) * span * 0.5
    p[..., 4] = rng.random((items, K2))
    p[..., 5] = rng.choice(labels, (items, K2))
    return p


LABEL_MAP = {1: 3, 2: 5, 3: 8, 5: 12, 6: 20}                  # label 4 has no category


# ---------------------------------------------------------------------------------------------- 1. layout
def check_layout(ops, device):
    rng = np.random.default_rng(0)
    packed = random_packed(rng, 6, 5)
    images = [Image(139, (1066, 800), (533, 400)), Image(285, (1066, 800), (640, 480))]       # equal ratios / different ratios
    assert images[0].rw == images[0].rh and images[1].rw != images[1].rh
    blocks = image_major(images, 3)
    assert [it for _, its in blocks for it in its] == [0, 2, 4, 1, 3, 5]
    for bit, want_over in ((1 << 16, 1), (0, 0)):
        counts = np.array([0, 5, 3 | bit, 0, 1, 5])
        for mode in ("lvis", "coco"):
            rows = check(ops, device, packed, counts, blocks, mode, label_map=LABEL_MAP)
            assert len(rows) == 14 and statement(packed, counts, blocks, mode, label_map=LABEL_MAP)[1] == want_over
    # candidate mode: plain counts, no overflow bit
    check(ops, device, packed, np.array([0, 5, 3, 0, 1, 5]), blocks, "lvis", candidate=True)


# ---------------------------------------------------------------------------------------------- 2. widths of the machine
def check_widths(ops, device):
    rng = np.random.default_rng(1)
    img = lambda n: Image(100 + n, (1333, 800), (640, 427))                              # noqa: E731
    packed = random_packed(rng, 4, 70)
    for mode in ("lvis", "coco"):
        check(ops, device, packed, np.array([70, 0, 69, 1]), image_major([img(0), img(1)], 2), mode, label_map=LABEL_MAP)
    packed = random_packed(rng, 130, 3)
    counts = rng.integers(0, 4, 130)
    counts[40:52] = 0                                                                    # whole images without a detection among them
    for mode, per in (("lvis", 2), ("coco", 2), ("coco", 130), ("coco", 1)):
        blocks = [(img(n), list(range(n * per, (n + 1) * per))) for n in range(130 // per)]
        check(ops, device, packed, counts, blocks, mode, label_map=LABEL_MAP)
    packed = random_packed(rng, 1, 4)
    for mode in ("lvis", "coco"):
        check(ops, device, packed, np.array([3]), [(img(0), [0])], mode, label_map=LABEL_MAP)
    packed, zero = random_packed(rng, 6, 4), np.zeros(6, np.int64)
    assert len(check(ops, device, packed, zero, image_major([img(0), img(1), img(2)], 2), "lvis")) == 0
    rows = check(ops, device, packed, zero, [(img(n), [n]) for n in range(6)], "coco", label_map=LABEL_MAP)
    assert len(rows) == 6 and np.isnan(rows[:, 1]).all() and (rows[:, 7] == 1).all() and (rows[:, 0] == 100 + np.arange(6)).all()


# ---------------------------------------------------------------------------------------------- 3. contraction
def check_contraction(ops, device):
    rng = np.random.default_rng(7)
    packed = random_packed(rng, 4, 1024, span=1066.0)
    image = Image(7, (1066, 800), (640, 480))
    assert np.float32(image.rw) == np.float32(640 / 1066) and np.float32(image.rh) == np.float32(480 / 800)
    # the inputs can tell a contracted build from this one: x2 * r - fp32(x1 * r) with the product kept exact (an fma) rounds differently
    r = np.float32(image.rw)
    x1, x2 = packed[..., 0].reshape(-1), packed[..., 2].reshape(-1)
    plain = x2 * r - x1 * r
    fused = (x2.astype(np.float64) * np.float64(r) - (x1 * r).astype(np.float64)).astype(np.float32)
    assert plain.dtype == np.float32 and np.count_nonzero(plain != fused) > len(plain) // 4, np.count_nonzero(plain != fused)
    blocks = [(image, [0, 1, 2, 3])]
    for mode in ("lvis", "coco"):
        rows = check(ops, device, packed, np.full(4, 1024), blocks, mode, label_map=LABEL_MAP)
        assert len(rows) == 4096


# ---------------------------------------------------------------------------------------------- 4. label table
def check_label_table(ops, device):
    rng = np.random.default_rng(3)
    packed = random_packed(rng, 4, 9, labels=(1, 2, 3, 4, 5, 6, 7, 40))
    counts = np.array([9, 4, 0, 7])
    blocks = image_major([Image(1, (100, 100), (100, 100)), Image(2, (100, 80), (200, 120))], 2)
    rows = check(ops, device, packed, counts, blocks, "coco", label_map=LABEL_MAP)
    lost = np.isin(np.concatenate([packed[it, :counts[it], 5] for _, its in blocks for it in its]), [4, 7, 40])
    assert lost.any() and not lost.all() and np.array_equal(np.isnan(rows[:, 1]), lost)               # NaN rows keep their place
    rows = check(ops, device, packed, counts, blocks, "coco", label_map={})
    assert len(rows) == 20 and np.isnan(rows[:, 1]).all()


# ---------------------------------------------------------------------------------------------- 5. bad inputs
def check_bad_inputs(ops, device, guarded=None):
    """guarded: a context manager factory under which the launches run once more with buffers of exactly the capacity (guard pages on the
    CPU, poison halos on the GPU)"""
    rng = np.random.default_rng(5)
    K2 = 6
    packed = random_packed(rng, 4, K2)
    blocks = image_major([Image(1, (100, 100), (50, 50)), Image(2, (100, 100), (100, 70))], 2)
    for candidate, counts in ((False, np.array([K2 + 9, 2, 0x1FFFF, 1])), (True, np.array([K2 + 9, 2, 70000, 1]))):
        for mode in ("lvis", "coco"):
            rows = check(ops, device, packed, counts, blocks, mode, candidate=candidate, label_map=LABEL_MAP)
            assert len(rows) == K2 + K2 + 2 + 1                               # the two bad counts read as K2
            if guarded is not None:
                with guarded():
                    check(ops, device, packed, counts, blocks, mode, candidate=candidate, label_map=LABEL_MAP, exact=True)
    # an entry that names an item the forward does not have is refused before any launch
    launched = []
    real = ops._chk
    ops._chk = lambda rc, name: (launched.append(name), real(rc, name))[1]
    try:
        for bad in (4, -1):
            try:
                ops.eval_rows_table([0, bad], [1.0, 1.0], [1.0, 1.0], [1.0, 1.0], [True, False], 4, device)
            except ValueError as e:
                assert f"item {bad}" in str(e)
            else:
                raise AssertionError("an entry naming a missing item was accepted")
        # ... and the entry point itself refuses a table that reaches it all the same (its host copy is checked, nothing is launched)
        table, host = ops.eval_rows_table([0, 1], [1.0, 1.0], [1.0, 1.0], [1.0, 1.0], [True, False], 4, device)
        host = host.clone()
        host[1, 0] = 4
        rows = torch.full((2 * K2, 7), FILL, dtype=torch.float32, device=device)
        state = torch.zeros(2, dtype=torch.int32, device=device)
        try:
            ops.eval_rows(torch.from_numpy(packed).to(device), torch.zeros(4, dtype=torch.int32, device=device), (table, host), rows, state)
        except RuntimeError as e:
            assert "mq_eval_rows failed with code -2" in str(e)
        else:
            raise AssertionError("mq_eval_rows accepted a table naming a missing item")
        assert launched == ["mq_eval_rows"] and bool((rows.cpu() == FILL).all())
        # too little room is refused by the wrapper
        table = ops.eval_rows_table([0, 1], [1.0, 1.0], [1.0, 1.0], [1.0, 1.0], [True, False], 4, device)
        try:
            ops.eval_rows(torch.from_numpy(packed).to(device), torch.zeros(4, dtype=torch.int32, device=device), table, rows[:2 * K2 - 1], state)
        except ValueError as e:
            assert "room" in str(e)
        else:
            raise AssertionError("a row buffer below the capacity was accepted")
    finally:
        ops._chk = real


# ---------------------------------------------------------------------------------------------- 6. accumulator
def check_accumulator(device):
    g = torch.Generator().manual_seed(2)
    for cls, cols in ((_ResultRows, 8), (FixedAPAccumulator, 7)):
        acc = cls(device) if cls is _ResultRows else cls(topk=1000, device=device)
        parts = []

        def block(cap, n):
            buf = torch.rand(cap, cols, generator=g).to(device)
            acc.append_block(buf, torch.tensor(n, dtype=torch.int32, device=device))
            parts.append(buf[:n])

        def plain(n):
            r = torch.rand(n, cols, generator=g).to(device)
            if cls is _ResultRows:
                acc.append(r)
            else:
                acc.update(r[:, 0], r[:, 1], r[:, 2], r[:, 3:])
            parts.append(r)
        block(10, 4)
        plain(3)
        block(6, 0)
        block(5, 5)
        plain(2)
        reads = []
        real = torch.Tensor.tolist
        torch.Tensor.tolist = lambda self: (reads.append(self.shape), real(self))[1]
        try:
            acc._fold()
        finally:
            torch.Tensor.tolist = real
        assert reads == [torch.Size([3])], reads                               # the three pending counts in one read
        want = torch.cat(parts)
        assert len(want) == 14
        if cls is FixedAPAccumulator:
            want = acc._prune(want)
        assert torch.equal(acc.rows.view(torch.int32), want.view(torch.int32)) and not acc._pending
        # the prune trigger weighs a block at its capacity
        acc = cls(device) if cls is _ResultRows else cls(topk=1000, device=device, prune_at=16)
        acc.prune_at = 16
        acc.append_block(torch.rand(10, cols, generator=g).to(device), torch.tensor(1, dtype=torch.int32, device=device))
        assert len(acc._pending) == 1 and len(acc.rows) == 0
        acc.append_block(torch.rand(6, cols, generator=g).to(device), torch.tensor(2, dtype=torch.int32, device=device))
        assert not acc._pending and len(acc.rows) == 3
    try:
        _ResultRows(device).append_block(torch.zeros(3, 7, device=device), torch.tensor(1, dtype=torch.int32, device=device))
    except ValueError:
        pass
    else:
        raise AssertionError("a block of another width was accepted")


def check_no_host_sync(device):
    """`update_packed` of both evaluators under torch's sync debug mode "error" (GPU only).  -> False when this torch build does not raise
    on a deliberate `.item()` under that mode: the assertion is then not made (the calls still run)."""
    rng = np.random.default_rng(9)
    packed = torch.from_numpy(random_packed(rng, 6, 5)).to(device)
    counts = torch.tensor([0, 5, 3 | 1 << 16, 0, 1, 5], dtype=torch.int32, device=device)
    lv = LvisFixedAPEvaluator(dict(LVIS_GT, annotations=[]), device=device)
    co = CocoAPEvaluator(dict(COCO_GT, annotations=[]), device=device)
    sizes = [(300, 380), (308, 390)]

    def calls(ids):
        lv.update_packed(packed, counts, ids, [(160, 192)] * 2, sizes, 3)
        co.update_packed(packed, counts, ids, [(160, 192)] * 2, None, 3)
    calls([11, 12])                                            # library load, pinned staging memory: once per process
    torch.cuda.synchronize()
    one = torch.ones(1, device=device)
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            one.item()
            raises = False
        except RuntimeError:
            raises = True
        if raises:
            calls([13, 14])
            calls([11, 12])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not raises:
        print("torch.cuda.set_sync_debug_mode('error') does not raise on .item() in this build: the no-sync assertion is not made")
        calls([13, 14])
        calls([11, 12])
    for ev, cols in ((lv, 7), (co, 8)):
        assert len(ev.acc._pending) == 3 and ev.acc._npending == 3 * (30 + (2 if cols == 8 else 0))
        ev.acc._fold()
        assert len(ev.acc.rows) == 3 * 14 and ev.tie_overflow()
    return raises


# ---------------------------------------------------------------------------------------------- 7. evaluators end to end
def pack_images(dets, K2=None):
    """dets[b] = [n_b, 6] fp32 rows of image b -> (packed [2 * B, K2, 6], raw counts [2 * B]) with every image's rows cut into two chunks
    (chunk-major items), the second item of the block carrying the tie-overflow bit"""
    B = len(dets)
    halves = [(d[:(len(d) + 1) // 2], d[(len(d) + 1) // 2:]) for d in dets]
    K2 = max([1] + [len(h) for pair in halves for h in pair]) if K2 is None else K2
    packed = np.full((2 * B, K2, 6), 3.0e4, np.float32)                        # dead slots hold no zero: a row of them would show
    counts = np.zeros(2 * B, np.int64)
    for b, pair in enumerate(halves):
        for c, h in enumerate(pair):
            packed[c * B + b, :len(h)] = h
            counts[c * B + b] = len(h)
    return packed, counts


def lvis_fixture(device):
    import test_lvis_eval_cpu as tl
    js, a = tl.load_case("small")
    preds = tl.predictions(js, a)
    ev = LvisFixedAPEvaluator(js["gt"], topk=js["topk"], device=device)
    for n in range(0, len(preds), 3):
        blk = preds[n:n + 3]
        dets = [torch.cat([p["boxes"].float(), p["scores"].float()[:, None], p["labels"].float()[:, None]], 1).numpy() for _, p in blk]
        packed, counts = pack_images(dets)
        sizes = [(480 + b, 640 + 2 * b) for b in range(len(blk))]              # ratio 1: the original size is the input size
        ev.update_packed(torch.from_numpy(packed).to(device), torch.from_numpy(counts.astype(np.int32)).to(device), [i for i, _ in blk],
                         sizes, sizes, 2)
    ev.synchronize_between_processes()
    strings = ev.summarize()
    want, want_strings = tl.run_case(js, a, device)
    assert strings == want_strings == js["strings"]
    for k in ("precision", "recall"):
        assert torch.equal(ev.eval[k], want.eval[k])
    assert np.array_equal(ev.eval["precision"].cpu().numpy(), a["precision"])
    same_rows(ev.acc.rows, want.acc.rows)
    assert not ev.tie_overflow()


def coco_fixture(device):
    import test_coco_eval_cpu as tc
    js, a = tc.load_case("small")
    items = tc.items_of(js, a)
    ev = CocoAPEvaluator(js["gt"], device=device, label_to_cat_id=tc.label_map(js))
    preds = [tc.boxlist(it, device) for it in items]
    full = [p for p in preds if len(p[1])]
    ev.update({full[-1][0]: full[0][1]})                                       # through `update`; the packed block below replaces it
    for n in range(0, len(items), 3):
        blk = items[n:n + 3]
        dets = [np.concatenate([np.asarray(b, np.float32).reshape(-1, 4), np.asarray(s, np.float32).reshape(-1, 1),
                                np.asarray(l, np.float32).reshape(-1, 1)], 1) for _, _, b, s, l in blk]
        packed, counts = pack_images(dets)
        ev.update_packed(torch.from_numpy(packed).to(device), torch.from_numpy(counts.astype(np.int32)).to(device), [it[0] for it in blk],
                         [(it[1][1], it[1][0]) for it in blk], None, 2)
    ev.update([full[0]])                                                       # an image that came packed arrives again through `update`
    ev.synchronize_between_processes()
    strings = ev.summarize()
    want, want_strings = tc.run_case(js, a, device)
    assert strings == want_strings == js["strings"]
    for k in ("precision", "recall"):
        assert torch.equal(ev.eval[k], want.eval[k])
    tc.check_case(js, a, ev, strings)
    same_rows(ev.eval["rows"], want.eval["rows"])


# ---------------------------------------------------------------------------------------------- 8. the loop
CHUNKS = (["caption a", "caption b", "caption c"], [{1: [1]}, {2: [3, 4]}, {3: [6]}])
LVIS_GT = {"images": [{"id": i, "neg_category_ids": [], "not_exhaustive_category_ids": []} for i in (11, 12, 13, 14)],
           "categories": [{"id": c, "frequency": f} for c, f in ((1, "f"), (2, "c"), (3, "r"), (4, "f"), (5, "c"), (6, "f"))]}
COCO_GT = {"images": [{"id": i, "width": 380 + 10 * n, "height": 300 + 8 * n} for n, i in enumerate((11, 12, 13, 14))],
           "categories": [{"id": c, "name": f"c{c}"} for c in (3, 5, 8, 11, 12, 20)]}


class Dataset:
    id_to_img_map = {0: 11, 1: 12, 2: 13, 3: 14}


class Loader:
    """two batches of two images: targets as the LVIS dataset makes them (dicts of tensors; the original id is the target's), image ids as the
    COCO datasets number them (positions, mapped through dataset.id_to_img_map)"""
    dataset = Dataset()

    def __init__(self, images, ids=(11, 12, 13, 14)):
        self.batches = []
        for n in range(0, len(ids), 2):
            targets = [{"image_id": torch.tensor(i), "orig_size": torch.tensor([300 + 8 * (n + k), 380 + 10 * (n + k)])}
                       for k, i in enumerate(ids[n:n + 2])]
            self.batches.append((images, targets, [n, n + 1], None))

    def __iter__(self):
        return iter(self.batches)


def with_annotations(gt, rows, lvis):
    """ground truths near some of the rows [n, 7], so that the summaries are not all -1"""
    gt = json.loads(json.dumps(gt))
    gt["annotations"] = []
    cats = {c["id"] for c in gt["categories"]}
    for r in rows[::max(1, len(rows) // 12)]:
        if r[1] == r[1] and int(r[1]) in cats and r[5] > 1 and r[6] > 1:
            ann = {"id": len(gt["annotations"]) + 1, "image_id": int(r[0]), "category_id": int(r[1]),
                   "bbox": [float(r[3]) + 1, float(r[4]) - 1, float(r[5]), float(r[6])], "area": float(r[5]) * float(r[6])}
            ann.update({} if lvis else {"iscrowd": 0})
            gt["annotations"].append(ann)
    return gt


def run_loop(model, loader, make_evaluator, packed, chunks=None, **kw):
    ev = make_evaluator()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        score = evaluate_detection(model, loader, ev, chunks or CHUNKS, device=ev.device, packed=packed, **kw)
    ev.acc._fold()
    return ev, score, [str(w.message) for w in caught]


def check_loop(model, images, device, expect_overflow=None, chunks=None):
    """`evaluate_detection` packed and through BoxLists: bit-equal rows, equal summaries, both evaluator kinds, one and several launch groups"""
    out = {}
    for lvis in (True, False):
        loader = Loader(images)
        plain = (lambda: LvisFixedAPEvaluator(dict(LVIS_GT, annotations=[]), device=device)) if lvis else \
            (lambda: CocoAPEvaluator(dict(COCO_GT, annotations=[]), device=device))
        probe, _, _ = run_loop(model, loader, plain, False, chunks)                    # a first run to place ground truths near the detections
        assert len(probe.acc.rows) > 0
        gt = with_annotations(LVIS_GT if lvis else COCO_GT, probe.acc.rows[:, :7].cpu().numpy(), lvis)
        assert gt["annotations"]
        make = (lambda gt=gt: LvisFixedAPEvaluator(gt, device=device)) if lvis else (lambda gt=gt: CocoAPEvaluator(gt, device=device))
        for kw in ({"max_items": 4}, {}):                                      # max_items 4: the three chunks of a batch in two launch groups
            # (the BoxList run at the same max_items: the model's own numbers depend on how many items a launch stacks)
            base, base_score, base_warn = run_loop(model, loader, make, False, chunks, **kw)
            assert base_score and any(not s.endswith("-1.000") for s in base_score)
            for mode in (True, "auto"):
                ev, score, warn = run_loop(model, loader, make, mode, chunks, **kw)
                same_rows(ev.acc.rows, base.acc.rows)
                assert score == base_score and torch.equal(ev.eval["precision"], base.eval["precision"])
                if expect_overflow is not None:
                    assert (TIE_OVERFLOW_WARNING in warn) == expect_overflow and warn.count(TIE_OVERFLOW_WARNING) <= 1, warn
                    assert any(TIE_OVERFLOW_WARNING in w for w in base_warn) == expect_overflow
        assert {int(i) for i in base.acc.rows[:, 0].tolist()} == {11, 12, 13, 14}
        # TEST.SUBSET counts batches
        model.cfg.TEST.SUBSET = 1
        try:
            for mode in (True, False):
                ev, _, _ = run_loop(model, loader, make, mode, chunks)
                assert {int(i) for i in ev.acc.rows[:, 0].tolist()} == {11, 12}
        finally:
            model.cfg.TEST.SUBSET = -1
        out["lvis" if lvis else "coco"] = (base, base_score, make, loader, chunks or CHUNKS)
    return out


def check_loop_refusals(model, images, device, chunks=CHUNKS):
    ev = LvisFixedAPEvaluator(dict(LVIS_GT, annotations=[]), device=device)
    model.cfg.VISION_QUERY.RETURN_ATTN_GATE_VALUE = True
    try:
        evaluate_detection(model, Loader(images), ev, chunks, device=device)
    except NotImplementedError as e:
        assert "RETURN_ATTN_GATE_VALUE" in str(e)
    else:
        raise AssertionError("RETURN_ATTN_GATE_VALUE was accepted")
    finally:
        model.cfg.VISION_QUERY.RETURN_ATTN_GATE_VALUE = False

    class NoPacked:
        def __init__(self, m):
            self.m, self.cfg = m, m.cfg

        def eval(self):
            return self

        def forward_chunks(self, *a, **k):
            return self.m.forward_chunks(*a, **k)
    try:
        evaluate_detection(NoPacked(model), Loader(images), ev, chunks, device=device, packed=True)
    except ValueError as e:
        assert "forward_chunks_packed" in str(e)
    else:
        raise AssertionError("packed=True on a model without forward_chunks_packed was accepted")
    assert len(ev.acc.rows) == 0 and not ev.acc._pending
    # ... while "auto" takes the BoxList path on such a model
    evaluate_detection(NoPacked(model), Loader(images), ev, chunks, device=device, packed="auto")
    ev.acc._fold()
    assert len(ev.acc.rows) > 0


WRITE_LINES = [" Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets= -1 catIds=all] = 0.250",
               " Average Recall     (AR) @[ IoU=0.50:0.95 | area= small | maxDets= -1 catIds=all] = -1.000"]
WRITE_TEXT = ("metric, avg \n"
              " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets= -1 catIds=all], 0.250 \n"
              " Average Recall     (AR) @[ IoU=0.50:0.95 | area= small | maxDets= -1 catIds=all], -1.000 \n")


def check_writers(tmp_path, device):
    """write_results = write_lvis_results (engine/inference.py:354-366), save_instances_results = lvis_eval.py:877-884"""
    path = os.path.join(str(tmp_path), "bbox.csv")
    LvisFixedAPEvaluator.write_results(WRITE_LINES, path)
    with open(path) as f:
        assert f.read() == WRITE_TEXT
    ev = LvisFixedAPEvaluator(dict(LVIS_GT, annotations=[]), device=device)
    ev.update([(12, {"scores": torch.tensor([0.5, 0.75]), "labels": torch.tensor([2, 1]), "boxes": torch.tensor([[1., 2., 4., 8.], [0., 0., 2., 2.]])}),
               (11, {"scores": torch.tensor([0.25]), "labels": torch.tensor([2]), "boxes": torch.tensor([[3., 3., 5., 6.]])})])
    path = os.path.join(str(tmp_path), "instances.json")
    ev.save_instances_results(path)
    with open(path) as f:
        got = json.load(f)
    assert got == [{"image_id": 11, "category_id": 2, "bbox": [3.0, 3.0, 2.0, 3.0], "score": 0.25},
                   {"image_id": 12, "category_id": 1, "bbox": [0.0, 0.0, 2.0, 2.0], "score": 0.75},
                   {"image_id": 12, "category_id": 2, "bbox": [1.0, 2.0, 3.0, 6.0], "score": 0.5}]


def check_loop_outputs(model, images, device, tmp_path, loops):
    """bbox.csv and TEST.LVIS_RESULTS_SAVE_PATH from the loop"""
    base, base_score, make, loader, chunks = loops["lvis"]
    csv, inst = os.path.join(str(tmp_path), "lvis.csv"), os.path.join(str(tmp_path), "lvis_instances.json")
    model.cfg.TEST.LVIS_RESULTS_SAVE_PATH = inst
    try:
        ev = make()
        score = evaluate_detection(model, loader, ev, chunks, device=device, output_file=csv)
    finally:
        model.cfg.TEST.LVIS_RESULTS_SAVE_PATH = ""
    assert score == base_score
    with open(csv) as f:
        text = f.read().split("\n")
    assert text[0] == "metric, avg " and len(text) == len(score) + 2 and text[1] == " ".join(score[0].split(" ")[:-2]) + ", " + score[0].split(" ")[-1] + " "
    with open(inst) as f:
        got = json.load(f)
    assert len(got) == len(ev.acc.rows) and [d["image_id"] for d in got] == sorted(d["image_id"] for d in got)
    base, base_score, make, loader, chunks = loops["coco"]
    csv = os.path.join(str(tmp_path), "coco.csv")
    score = evaluate_detection(model, loader, make(), chunks, device=device, output_file=csv)
    with open(csv) as f:
        assert f.read() == "\n".join(base_score) + "\n" and score == base_score


# ---------------------------------------------------------------------------------------------- a stand-in model (no GPU)
class StubModel:
    """`forward_chunks_packed` returns canned blocks, `forward_chunks` the `_boxlists` of the same blocks: what the real model's two calls
    are to each other"""

    def __init__(self, device, overflow=False, seed=11):
        self.cfg = get_cfg()
        self.device = torch.device(device)
        self.overflow, self.seed = overflow, seed
        self.last_tie_overflow = []

    def eval(self):
        return self

    def _blocks(self, images, chunks, max_items):
        B = images.tensors.shape[0]
        rng = np.random.default_rng(self.seed)
        K2, per = 7, max(1, int(max_items) // B)
        packed = random_packed(rng, len(chunks) * B, K2, span=150.0)
        counts = rng.integers(0, K2 + 1, len(chunks) * B)
        counts[1] = 0
        if self.overflow:
            counts[2] |= 1 << 16
        out = []
        for g0 in range(0, len(chunks), per):
            g = len(chunks[g0:g0 + per])
            sl = slice(g0 * B, (g0 + g) * B)
            out.append((torch.from_numpy(packed[sl]).to(self.device), torch.from_numpy(counts[sl].astype(np.int32)).to(self.device), g))
        return out

    def forward_chunks_packed(self, images, chunks, max_items=32):
        return self._blocks(images, chunks, max_items)

    _split_counts = GeneralizedVLRCNN_New._split_counts

    def forward_chunks(self, images, chunks, max_items=32):
        B = images.tensors.shape[0]
        results = []
        for packed, counts, g in self._blocks(images, chunks, max_items):
            counts = self._split_counts(counts.tolist())
            for c in range(g):
                results.append(GeneralizedVLRCNN_New._boxlists(packed, counts, images.image_sizes, first=c * B))
        return results
