"""COCO AP on the MI355X (mq_det_amd.evaluation.CocoAPEvaluator, csrc/ap_eval.hip): the three fixtures of tests/test_coco_eval_cpu.py and the
pair above the fast path with the same exact comparisons, the same under the NaN poison halos of tests/halo.py, a 200-image x 20-category
random case against the restatement, and the engine's calls (per-image concatenation of forward_chunks' detections, update, the RCCL exchange
in a one-rank group, summarize) on detections of the tiny MQ-GLIP model.  No time is asserted (tools/coco_eval_bench.py measures)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.dirname(HERE))

import coco_eval_ref as ref  # noqa: E402
import test_coco_eval_cpu as tc  # noqa: E402
from mq_det_amd.evaluation import CocoAPEvaluator  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("name", ["bridge", "small", "medium"])
def test_fixture_on_device_is_exact(name):
    js, a = tc.load_case(name)
    ev, strings = tc.run_case(js, a, DEV)
    assert ev.eval["precision"].is_cuda and ev.acc.rows.is_cuda
    tc.check_case(js, a, ev, strings)


def test_big_pair_on_device_matches_the_restated_evaluate_img():
    tc.check_big_pair(DEV)


def test_fixtures_and_big_pair_under_nan_halos():
    from halo import poisoned_args
    for name in ("bridge", "small", "medium"):
        js, a = tc.load_case(name)
        with poisoned_args("nan"):
            ev, strings = tc.run_case(js, a, DEV)
        tc.check_case(js, a, ev, strings)
    with poisoned_args("nan"):
        tc.check_big_pair(DEV)


def test_random_200_images_20_categories_match_the_restatement():
    ev = tc.check_random_case(DEV, 200, 20)
    assert len(ev.eval["rows"]) > 5000 and ev.eval["pair_gt"][:, 1].max().item() >= 2


def test_engine_calls_on_forward_chunks_detections():
    """CocoAPEvaluator as engine/inference.py's COCO branch uses the detections: forward_chunks (tiny model, two images, three chunk captions),
    the chunks' BoxLists concatenated per image, update, synchronize_between_processes(force=True) over RCCL, summarize -- against the
    restatement fed the same boxes."""
    import torch.distributed as dist
    import parity_checks as pc
    from mq_det_amd.structures import ImageList, cat_boxlist
    created = False
    if not dist.is_initialized():
        with socket.socket() as s_:
            s_.bind(("127.0.0.1", 0))
            port = s_.getsockname()[1]
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1)
        created = True
    try:
        spec, sd, cfg, model, P = pc.tiny(DEV)
        images, sizes, ids, am, pm, bank = pc.make_inputs(spec)
        model.load_query_bank(bank)
        kv = int(am[0].sum())
        model.tokenize = lambda caps, dev: (ids[:1].expand(len(caps), -1).contiguous().to(dev), am[:1].expand(len(caps), -1).contiguous().to(dev), kv)
        image_ids = [139, 285]
        with torch.no_grad():
            outs = model.forward_chunks(ImageList(images.to(DEV), sizes), [("caption a", pm), ("caption b", pm), ("caption c", pm)])
        per_image = {i: cat_boxlist([out[b] for out in outs]) for b, i in enumerate(image_ids)}          # engine/inference.py:643-650
        cat_ids = [3, 5, 8, 11, 12, 20]
        gt = {"images": [{"id": i, "width": 2 * per_image[i].size[0], "height": 3 * per_image[i].size[1] // 2} for i in image_ids],
              "categories": [{"id": c, "name": f"c{c}"} for c in cat_ids], "annotations": []}
        items = [(i, per_image[i].size, per_image[i].bbox.cpu().numpy(), per_image[i].get_field("scores").float().cpu().numpy(),
                  per_image[i].get_field("labels").cpu().numpy()) for i in image_ids]
        rows = ref.result_rows(items, gt)
        g = np.random.default_rng(4)
        for j in g.choice(len(rows), min(len(rows), 24), replace=False):        # ground truths near some of the detections, a crowd among them
            x, y, w, h = rows[j, 3:7] + g.normal(0, 2, 4)
            if w > 1 and h > 1:
                gt["annotations"].append({"id": len(gt["annotations"]) + 1, "image_id": int(rows[j, 0]), "category_id": int(rows[j, 1]),
                                          "bbox": [float(x), float(y), float(w), float(h)], "area": float(w * h),
                                          "iscrowd": int(len(gt["annotations"]) == 5)})
        ev = CocoAPEvaluator(gt, device=DEV)
        ev.update(per_image)
        ev.synchronize_between_processes(force=True)
        strings = ev.summarize()
        out = ref.evaluate(gt, rows)
        assert len(rows) > 0 and len(ev.eval["rows"]) > 0 and (out["precision"] > 0).any()
        assert np.array_equal(ev.eval["precision"].cpu().numpy(), out["precision"]) and np.array_equal(ev.eval["recall"].cpu().numpy(), out["recall"])
        assert strings == out["strings"] and all(abs(x - y) <= 1e-12 for x, y in zip(ev.stats, out["stats"]))
    finally:
        if created:
            dist.destroy_process_group()
