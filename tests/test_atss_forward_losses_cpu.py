"""`forward_losses` end to end without a GPU: the tiny MQ-GLIP of the parity ladders with fp32 operands, every kernel SOURCE through the
host emulation (the fixture of tests/test_simt_fp32_operands_cpu.py: the precise mode exactly as the device launches it), against the fp32
oracle's head outputs fed to the from-scratch restatement of tests/atss_loss_ref.py.  Assignment and num_pos equal, each loss within the
project's standing gate 1e-3 + 1e-3 |ref|."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import atss_loss_cases as ac  # noqa: E402
from test_simt_fp32_operands_cpu import _CXX, f32  # noqa: E402,F401

pytestmark = pytest.mark.skipif(not os.path.exists(_CXX), reason=f"{_CXX} not found: the kernel-source emulation cannot be built here")


def test_forward_losses_on_the_tiny_model_meets_1e_3(f32):
    out, want = ac.end_to_end(torch.device("cpu"), torch.float32, switch=False)
    for b, m in enumerate(want["matched"]):
        assert torch.equal(out["matched"][b].long(), m), b
    assert int(out["sums"][0]) == want["num_pos"] > 0 and float(out["loss_cls"]) == 0.0
    for k in ("loss_reg", "loss_centerness", "loss_dot_product_token"):
        print("atss_loss end_to_end emulation float32", k, float(out[k]), want[k])
        assert abs(float(out[k]) - want[k]) <= 1e-3 + 1e-3 * abs(want[k]), (k, float(out[k]), want[k])
