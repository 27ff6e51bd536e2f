"""world-2 gloo worker: tensor evaluator gather (mq_det_amd.evaluation) vs what the reference's own LvisEvaluatorFixedAP +
utils/mdetr_dist.all_gather (pickle all_gather on the CPU group) return for the same per-rank inputs -- recorded by
oracle/gen_golden_dropin.py in tests/golden/dropin_reference.json."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOPK = 7


def rank_annotations(rank):
    """Six "images" per rank, 30 detections each, 5 categories, score ties: one list of LVIS-style annotations per image."""
    g = torch.Generator().manual_seed(100 + rank)
    out = []
    for it in range(6):
        n = 30
        img = 1000 * rank + it
        labels = torch.randint(1, 6, (n,), generator=g)
        scores = (torch.randint(0, 50, (n,), generator=g).float() / 50.0)
        boxes = torch.rand(n, 4, generator=g) * 100
        out.append([{"image_id": img, "category_id": int(labels[k]), "bbox": boxes[k].tolist(), "score": float(scores[k])} for k in range(n)])
    return out


def main():
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    from mq_det_amd import parallel
    from mq_det_amd.evaluation import FixedAPAccumulator

    rank, local, world = parallel.init_distributed("gloo")
    assert world == 2
    with open(os.path.join(ROOT, "tests", "golden", "dropin_reference.json")) as f:
        ref_by_cat = {int(c): v for c, v in json.load(f)["evaluator"]["world2_synchronized"].items()}
    acc = FixedAPAccumulator(topk=TOPK, prune_at=40)
    for anns in rank_annotations(rank):
        acc.update(torch.tensor([float(a["image_id"]) for a in anns]), torch.tensor([a["category_id"] for a in anns]),
                   torch.tensor([a["score"] for a in anns]), torch.tensor([a["bbox"] for a in anns]))
    acc.synchronize_between_processes()
    mine = acc.by_cat()
    assert set(mine) == set(ref_by_cat), (set(mine), set(ref_by_cat))
    for cat, anns in ref_by_cat.items():
        a = [(i, round(s, 6), [round(v, 3) for v in b]) for i, s, b in anns]
        b = [(x["image_id"], round(x["score"], 6), [round(v, 3) for v in x["bbox"]]) for x in mine[cat]]
        assert a == b, (cat, a[:3], b[:3])
        assert len(a) <= 2 * TOPK
    dist.barrier()
    print("EVAL_GATHER_OK", rank, sum(len(v) for v in mine.values()), flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
