"""The match / accumulate kernels both AP evaluators share (csrc/ap_eval.hip; mq_det_amd.ops lvis_* / coco_*) on the MI355X: the checks of
tests/ap_eval_checks.py with the kernels themselves, exact on the bits."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.dirname(HERE))

import ap_eval_checks as ac  # noqa: E402
from mq_det_amd import ops  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]
DEV = torch.device("cuda:0")


def test_rule_sets_coincide_without_crowd_ignore_and_not_exhaustive():
    ac.check_rule_sets_coincide(ops, DEV)


@pytest.mark.parametrize("rules,n_gt", [("lvis", ac.LVIS_FAST_GT), ("lvis", ac.LVIS_FAST_GT + 1), ("coco", ac.COCO_FAST_GT),
                                        ("coco", ac.COCO_FAST_GT + 1)])
def test_both_sides_of_each_fast_path_bound(rules, n_gt):
    ac.check_fast_path_bound(ops, DEV, rules, n_gt)


def test_coco_max_dets_slices():
    ac.check_max_dets_slices(ops, DEV)
