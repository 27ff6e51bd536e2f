"""world-2 gloo worker: the normalisers of mq_det_amd.losses.ATSSLoss.losses_from_sums.  Each rank holds its own raw sums (rank 1 has no
positives); the losses must be the local sums over max(total positives / world, 1) and (total centerness / world), the reference's
reduce_sum rule (rpn/loss.py:1147-1191)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    from mq_det_amd import get_cfg, parallel
    from mq_det_amd.losses import ATSSLoss

    rank, local, world = parallel.init_distributed("gloo")
    assert world == 2
    # num_pos, S ct, S ct (1 - GIoU), S BCE, S (1 - GIoU), S token
    raw = [torch.tensor([5.0, 3.0, 2.0, 4.0, 3.5, 90.0]), torch.tensor([0.0, 0.0, 0.0, 0.0, 0.0, 40.0])]
    crit = ATSSLoss(get_cfg())
    out = crit.losses_from_sums(raw[rank])
    npos_avg, ct_avg = max((5.0 + 0.0) / 2, 1.0), (3.0 + 0.0) / 2
    want = [{"loss_reg": 2.0 * 2.0 / ct_avg, "loss_centerness": 4.0 / npos_avg, "loss_dot_product_token": 90.0 / npos_avg},
            {"loss_reg": 0.0, "loss_centerness": 0.0, "loss_dot_product_token": 40.0 / npos_avg}][rank]
    for k, v in want.items():
        assert abs(float(out[k]) - v) <= 1e-6 * max(1.0, abs(v)), (rank, k, float(out[k]), v)
    assert float(out["loss_cls"]) == 0.0
    # fewer positives than ranks: the floor of 1
    out = crit.losses_from_sums(torch.tensor([1.0, 0.5, 0.25, 1.0, 0.5, 8.0]) * (rank == 0))
    if rank == 0:
        assert abs(float(out["loss_centerness"]) - 1.0) <= 1e-6 and abs(float(out["loss_reg"]) - 2.0 * 0.25 / 0.25) <= 1e-6
    dist.barrier()
    print("ATSS_NORMALISERS_OK", rank, flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
