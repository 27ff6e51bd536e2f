"""`GroundingDINO.forward_losses` end to end without a GPU: the shallow MQ-GroundingDINO of the parity ladders with fp32 operands, every kernel
SOURCE through the host emulation (the fixture of tests/test_simt_fp32_operands_cpu.py), against the aux outputs built from the `hs` / `refs`
of the fp32 oracle's trace.  Per-layer logits and boxes within 1e-3 + 1e-3 |ref|; the device's assignment optimal within 2 G eps on its own
outputs; the losses within the standing gate of the restatement's for the device's assignment; loss_gate from the ff_gate parameters."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import set_loss_cases as sc  # noqa: E402
from test_simt_fp32_operands_cpu import _CXX, f32  # noqa: E402,F401

pytestmark = pytest.mark.skipif(not os.path.exists(_CXX), reason=f"{_CXX} not found: the kernel-source emulation cannot be built here")


def test_forward_losses_on_the_tiny_model_meets_1e_3(f32):
    if f32._f32_mode == 2:
        pytest.skip("same launches as under device_limits")
    out, want = sc.end_to_end(torch.device("cpu"))
    assert set(out) >= {"loss_ce", "loss_bbox", "loss_giou", "loss_ce_0", "loss_bbox_0", "loss_giou_0", "loss_gate", "sums", "match_q", "q2g"}
    sc.check_end_to_end(out, want)
