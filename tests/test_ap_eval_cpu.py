"""The match / accumulate kernels both AP evaluators share (csrc/ap_eval.hip; mq_det_amd.ops lvis_* / coco_*) without a GPU: the kernel SOURCE
through the host emulation (tests/simt) on the hand-made inputs of tests/ap_eval_checks.py -- where LVIS's and COCO's rules coincide the two
instantiations agree bit for bit and equal the restatement; each keeps its own fast-path bound; COCO's maxDets slices."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ap_eval_checks as ac  # noqa: E402

_CXX = os.environ.get("SIMT_CXX", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not os.path.exists(_CXX), reason=f"{_CXX} not found: the kernel-source emulation cannot be built here")


@pytest.fixture(scope="module")
def emu():
    import simt
    with simt.installed() as ops:
        yield ops


def test_rule_sets_coincide_without_crowd_ignore_and_not_exhaustive(emu):
    ac.check_rule_sets_coincide(emu, "cpu")


@pytest.mark.parametrize("rules,n_gt", [("lvis", ac.LVIS_FAST_GT), ("lvis", ac.LVIS_FAST_GT + 1), ("coco", ac.COCO_FAST_GT),
                                        ("coco", ac.COCO_FAST_GT + 1)])
def test_both_sides_of_each_fast_path_bound(emu, rules, n_gt):
    ac.check_fast_path_bound(emu, "cpu", rules, n_gt)


def test_coco_max_dets_slices(emu):
    ac.check_max_dets_slices(emu, "cpu")
