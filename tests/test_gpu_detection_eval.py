"""The detection evaluation loop on the MI355X (mq_det_amd.detection.evaluate_detection, the evaluators' `update_packed`, csrc/eval_rows.hip):
the checks of tests/detection_eval_checks.py with the kernel itself -- the rows against their numpy fp32 statement on the bits (layout,
widths, contraction, label table, bad counts, the last also under the NaN poison halos of tests/halo.py), no host sync inside `update_packed`,
both evaluators end to end on the small fixtures, and the loop packed against BoxLists on the tiny MQ-GLIP model.  No time is asserted
(tools/detection_eval_bench.py measures)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.dirname(HERE))

import detection_eval_checks as dc  # noqa: E402
from mq_det_amd import ops  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]
DEV = torch.device("cuda:0")


def test_layout_permutation_and_overflow_flag():
    dc.check_layout(ops, DEV)


def test_rows_across_lanes_waves_and_empty_images():
    dc.check_widths(ops, DEV)


def test_widths_are_not_contracted():
    dc.check_contraction(ops, DEV)


def test_label_table():
    dc.check_label_table(ops, DEV)


def test_bad_counts_stay_inside_the_buffer_and_bad_items_are_refused():
    from halo import poisoned_args
    dc.check_bad_inputs(ops, DEV, guarded=lambda: poisoned_args("nan"))


def test_accumulator_keeps_blocks_whole_and_reads_their_counts_once():
    dc.check_accumulator(DEV)


def test_update_packed_does_not_sync_the_host():
    dc.check_no_host_sync(DEV)


def test_lvis_fixture_through_update_packed():
    dc.lvis_fixture(DEV)


def test_coco_fixture_through_update_packed_and_update_mixed():
    dc.coco_fixture(DEV)


@pytest.fixture(scope="module")
def tiny():
    """the tiny MQ-GLIP model with its query bank, two images, three chunk captions over the same token ids with different positive maps"""
    import parity_checks as pc
    from mq_det_amd.structures import ImageList
    spec, sd, cfg, model, P = pc.tiny(DEV)
    images, sizes, ids, am, pm, bank = pc.make_inputs(spec)
    model.load_query_bank(bank)
    kv = int(am[0].sum())
    saved = model.tokenize
    model.tokenize = lambda caps, dev: (ids[:1].expand(len(caps), -1).contiguous().to(dev), am[:1].expand(len(caps), -1).contiguous().to(dev), kv)
    chunks = (["caption a", "caption b", "caption c"], [pm, {k: pm[k] for k in (2, 5)}, {k: pm[k] for k in (1, 3, 4, 6)}])
    try:
        yield model, ImageList(images.to(DEV), sizes), chunks
    finally:
        model.tokenize = saved
        model.cfg.TEST.SUBSET = -1


def test_loop_packed_equals_boxlists_on_the_tiny_model(tiny, tmp_path):
    model, images, chunks = tiny
    loops = dc.check_loop(model, images, DEV, chunks=chunks)
    dc.check_writers(tmp_path, DEV)
    dc.check_loop_outputs(model, images, DEV, tmp_path, loops)


def test_loop_refusals_on_the_tiny_model(tiny):
    model, images, chunks = tiny
    dc.check_loop_refusals(model, images, DEV, chunks=chunks)
