"""world-2 gloo worker: the normaliser of mq_det_amd.set_loss.SetCriterionLoss.losses_from_sums.  Each rank holds its own raw sums and gt
count; the losses must be the local sums over max(total gts / world, 1) times the coefficients (loss.py:131-136, :166-171)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    from mq_det_amd import parallel
    from mq_det_amd.config import get_gdino_cfg
    from mq_det_amd.set_loss import SetCriterionLoss

    rank, local, world = parallel.init_distributed("gloo")
    assert world == 2
    sums = [torch.tensor([[90.0, 3.0, 2.0], [80.0, 2.5, 1.5]]), torch.tensor([[40.0, 0.0, 0.0], [30.0, 0.0, 0.0]])][rank]
    crit = SetCriterionLoss(get_gdino_cfg())
    out = crit.losses_from_sums(sums, [5, 0][rank])
    n = max((5 + 0) / 2, 1.0)
    for l, sfx in ((0, "_0"), (1, "")):
        for j, (name, c) in enumerate((("loss_ce", 2.0), ("loss_bbox", 5.0), ("loss_giou", 2.0))):
            want = float(sums[l, j]) / n * c
            assert abs(float(out[name + sfx]) - want) <= 1e-6 * max(1.0, abs(want)), (rank, name + sfx, float(out[name + sfx]), want)
    assert set(out) == {a + b for a in ("loss_ce", "loss_bbox", "loss_giou") for b in ("", "_0")}
    # fewer gts than ranks: the floor of 1
    out = crit.losses_from_sums(sums, [1, 0][rank])
    assert abs(float(out["loss_ce"]) - float(sums[1, 0]) * 2.0) <= 1e-4
    dist.barrier()
    print("SET_LOSS_NUM_BOXES_OK", rank, flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
