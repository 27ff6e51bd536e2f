"""The detection evaluation loop (mq_det_amd.detection.evaluate_detection, the evaluators' `update_packed`, csrc/eval_rows.hip) without a GPU:
the kernel SOURCE through the host emulation (tests/simt) against the rows stated in numpy fp32 in tests/detection_eval_checks.py -- layout and
permutation, the widths of the machine, contraction, the label table, bad counts under the buffer-overrun guard --, the accumulator's blocks,
both evaluators end to end on tests/golden/{lvis,coco}_eval_small, and the loop on a stand-in model."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import detection_eval_checks as dc  # noqa: E402

_CXX = os.environ.get("SIMT_CXX", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not os.path.exists(_CXX), reason=f"{_CXX} not found: the kernel-source emulation cannot be built here")


@pytest.fixture(scope="module")
def emu():
    import simt
    with simt.installed() as ops:
        yield ops


@pytest.fixture(scope="module")
def images():
    return torch.zeros(2, 3, 160, 192)


def test_layout_permutation_and_overflow_flag(emu):
    dc.check_layout(emu, "cpu")


def test_rows_across_lanes_waves_and_empty_images(emu):
    dc.check_widths(emu, "cpu")


def test_widths_are_not_contracted(emu):
    dc.check_contraction(emu, "cpu")


def test_label_table(emu):
    dc.check_label_table(emu, "cpu")


def test_bad_counts_stay_inside_the_buffer_and_bad_items_are_refused(emu):
    from simt import guard
    dc.check_bad_inputs(emu, "cpu", guarded=lambda: guard.pointer_guard("end"))


@pytest.mark.parametrize("schedule", [("descending", 0), ("random", 5)])
def test_layout_under_other_fibre_schedules(emu, schedule):
    import simt
    simt.set_schedule(*schedule)
    try:
        dc.check_layout(emu, "cpu")
        dc.check_widths(emu, "cpu")
    finally:
        simt.set_schedule("ascending")


def test_accumulator_keeps_blocks_whole_and_reads_their_counts_once(emu):
    dc.check_accumulator("cpu")


def test_lvis_fixture_through_update_packed(emu):
    dc.lvis_fixture("cpu")


def test_coco_fixture_through_update_packed_and_update_mixed(emu):
    dc.coco_fixture("cpu")


@pytest.mark.parametrize("overflow", [False, True])
def test_loop_packed_equals_boxlists(emu, images, overflow):
    dc.check_loop(dc.StubModel("cpu", overflow=overflow), images, "cpu", expect_overflow=overflow)


def test_loop_refusals(emu, images):
    dc.check_loop_refusals(dc.StubModel("cpu"), images, "cpu")


def test_result_writers_and_loop_outputs(emu, images, tmp_path):
    dc.check_writers(tmp_path, "cpu")
    model = dc.StubModel("cpu")
    dc.check_loop_outputs(model, images, "cpu", tmp_path, dc.check_loop(model, images, "cpu"))
