"""LVIS Fixed AP on the MI355X (mq_det_amd.evaluation.LvisFixedAPEvaluator, csrc/ap_eval.hip): both reference fixtures bit for bit, the same
under the NaN poison halos of tests/halo.py, one pair of more than 2 000 detections x 500 ground truths, the LVIS-minival shape (4 809 images,
1 203 categories, 50 000 ground truths, topk 10 000 = 12M rows), and the engine's calls on detections of forward_chunks.  Every test runs its
body in a process of its own under a time limit (a fault or a hang fails that test, not the session)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.dirname(HERE))

import lvis_eval_ref as ref  # noqa: E402
import test_lvis_eval_cpu as tc  # noqa: E402
from mq_det_amd.evaluation import LvisFixedAPEvaluator  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]
DEV = torch.device("cuda:0")


def _body_fixtures():
    for name in ("small", "medium"):
        js, a = tc.load_case(name)
        ev, strings = tc.run_case(js, a, DEV)
        assert ev.eval["precision"].is_cuda
        tc.check_case(name, ev, strings, flags=name == "small")
        print(f"OK {name}: {strings[0]}", flush=True)


def _body_fixtures_halo():
    from halo import poisoned_args
    for name in ("small", "medium"):
        js, a = tc.load_case(name)
        with poisoned_args("nan"):
            ev, strings = tc.run_case(js, a, DEV)
        tc.check_case(name, ev, strings, flags=name == "small")
    with poisoned_args("nan"):
        tc.check_big_pair(DEV)
    print("OK fixtures and the big pair under NaN halos", flush=True)


def _body_big_pair():
    tc.check_big_pair(DEV)
    print("OK big pair", flush=True)


def _minival(gt, rows, topk=10000):
    ev = LvisFixedAPEvaluator(gt, topk=topk, device=DEV)
    ev.acc.update(torch.from_numpy(rows[:, 0]), torch.from_numpy(rows[:, 1]), torch.from_numpy(rows[:, 2]), torch.from_numpy(rows[:, 3:]))
    ev.synchronize_between_processes()
    torch.cuda.synchronize()
    t0 = time.time()
    strings = ev.summarize()
    return ev, strings, time.time() - t0


def _body_minival():
    from mq_det_amd.utils.synth import synthetic_lvis
    gt, rows = synthetic_lvis()
    ev, strings, dt = _minival(gt, rows)
    P, R = ev.eval["precision"], ev.eval["recall"]
    n_rows, n_pairs = len(ev.acc.rows), len(ev.eval["pair_key"])
    print(f"minival: {n_rows} rows, {n_pairs} pairs, {int(ev.eval['pair_dt'][:, 1].sum())} detections evaluated, summarize {dt:.2f} s",
          flush=True)
    assert n_rows > 10_000_000 and not torch.isnan(P).any() and not torch.isnan(R).any()
    assert (P > 0).any()
    for s in strings:
        print(s, flush=True)
    # the categories evaluated as two disjoint halves: per-category precision / recall identical
    K = len(gt["categories"])
    for lo, hi in ((0, K // 2), (K // 2, K)):
        ids = {c["id"] for c in gt["categories"][lo:hi]}
        half = dict(gt, categories=gt["categories"][lo:hi], annotations=[a for a in gt["annotations"] if a["category_id"] in ids])
        eh, _, _ = _minival(half, rows)
        assert torch.equal(eh.eval["precision"], P[:, :, lo:hi]) and torch.equal(eh.eval["recall"], R[:, lo:hi]), (lo, hi)
    # 50 random pairs against the restated evaluate_img, all 4 areas
    g = np.random.default_rng(0)
    has = ((ev.eval["pair_dt"][:, 1] > 0) & (ev.eval["pair_gt"][:, 1] > 0)).nonzero()[:, 0].cpu().numpy()
    pick = ev.eval["pair_key"][torch.from_numpy(g.choice(has, 50, replace=False)).to(DEV)].cpu().tolist()
    img_ids, cat_ids = ev.img_ids_f.cpu().long().tolist(), ev.cat_ids_f.cpu().long().tolist()
    keys = [(img_ids[k // K], cat_ids[k % K]) for k in pick]
    got = tc.pair_flags(ev, keys)
    results = ev.acc._prune(ev.acc.rows)                 # _summarize_fixed's results, in order
    imgs = {im["id"]: im for im in gt["images"]}
    per_img = {}
    for a in gt["annotations"]:
        per_img.setdefault(a["image_id"], []).append(a)
    for i, c in keys:
        sel = results[(results[:, 0] == i) & (results[:, 1] == c)].cpu().tolist()
        dts = [(r[2], r[3:7], r[5] * r[6]) for r in sel if 0 < r[5] * r[6] < float("inf")]
        gts = [(a["id"], a["bbox"], a["area"], bool(a.get("ignore", 0))) for a in per_img.get(i, []) if a["category_id"] == c and 0 < a["area"]]
        m, ig, cnt = got[(i, c)]
        for ai, rng in enumerate(ref.AREA_RNG):
            wm, wi, gig, _ = ref.evaluate_img(dts, gts, rng, c in imgs[i]["not_exhaustive_category_ids"])
            assert np.array_equal(m[ai], wm) and np.array_equal(ig[ai], wi), (i, c, ai)
            assert cnt[ai] == int(np.count_nonzero(gig == 0)), (i, c, ai)
    print("OK minival: halves identical, 50 pairs match the restatement", flush=True)


def _body_engine():
    """LvisFixedAPEvaluator exactly as engine/inference.py uses it: update with mdetr_style_output items of forward_chunks (tiny model, two
    images, three chunk captions), synchronize_between_processes, summarize -- against the restated _summarize_fixed on the same by_cat()."""
    import parity_checks as pc
    from mq_det_amd.structures import ImageList
    spec, sd, cfg, model, P = pc.tiny(DEV)
    images, sizes, ids, am, pm, bank = pc.make_inputs(spec)
    model.load_query_bank(bank)
    kv = int(am[0].sum())
    model.tokenize = lambda caps, dev: (ids[:1].expand(len(caps), -1).contiguous().to(dev), am[:1].expand(len(caps), -1).contiguous().to(dev), kv)
    image_ids = [139, 285]
    with torch.no_grad():
        outs = model.forward_chunks(ImageList(images.to(DEV), sizes), [("caption a", pm), ("caption b", pm), ("caption c", pm)])
    g = np.random.default_rng(4)
    anns, images_js = [], []
    for b, i in enumerate(image_ids):                    # ground truths near some of the detections, so that every rule has work
        bx = outs[0][b].bbox.cpu().numpy()
        lb = outs[0][b].get_field("labels").cpu().numpy()
        for j in g.choice(len(bx), min(len(bx), 12), replace=False):
            x1, y1, x2, y2 = bx[j] + g.normal(0, 2, 4)
            if x2 > x1 and y2 > y1:
                anns.append({"id": len(anns) + 1, "image_id": i, "category_id": int(lb[j]), "bbox": [float(x1), float(y1), float(x2 - x1), float(y2 - y1)],
                             "area": float((x2 - x1) * (y2 - y1))})
        images_js.append({"id": i, "neg_category_ids": [1, 2, 3], "not_exhaustive_category_ids": [4]})
    gt = {"images": images_js, "annotations": anns, "categories": [{"id": c, "frequency": "rcf"[c % 3]} for c in range(1, 7)]}
    ev = LvisFixedAPEvaluator(gt, topk=40, device=DEV)
    for out in outs:                                     # one engine step per chunk: mdetr_style_output of the step's images
        step = [(i, {"scores": o.get_field("scores"), "labels": o.get_field("labels"), "boxes": o.bbox}) for i, o in zip(image_ids, out)]
        ev.update(step)
    ev.synchronize_between_processes()
    strings = ev.summarize()
    rows = np.asarray([[d["image_id"], d["category_id"], d["score"]] + d["bbox"] for lst in ev.acc.by_cat().values() for d in lst], np.float64)
    p, r, res, want, _ = ref.summarize_fixed(gt, rows, 40)
    assert np.array_equal(ev.eval["precision"].cpu().numpy(), p) and np.array_equal(ev.eval["recall"].cpu().numpy(), r)
    assert strings == want and all(abs(ev.results[k] - v) <= 1e-12 for k, v in res.items())
    assert len(rows) > 0 and (p > 0).any()
    print(f"OK engine path: {len(rows)} rows, {strings[0]}", flush=True)


def _run(body, timeout):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), body], capture_output=True, text=True, timeout=timeout)
    out = r.stdout + r.stderr
    assert r.returncode == 0, f"{body}: rc {r.returncode}\n{out[-4000:]}"
    return out


def test_fixtures_on_device_are_exact():
    _run("fixtures", 300)


def test_fixtures_and_big_pair_under_nan_halos():
    _run("fixtures_halo", 300)


def test_big_pair_on_device_matches_the_restated_evaluate_img():
    _run("big_pair", 300)


def test_lvis_minival_shape():
    print(_run("minival", 900)[-3000:])


def test_engine_calls_on_forward_chunks_detections():
    _run("engine", 600)


if __name__ == "__main__":
    globals()["_body_" + sys.argv[1]]()
