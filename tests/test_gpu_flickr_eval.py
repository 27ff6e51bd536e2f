"""Flickr30k Entities Recall@k on the MI355X (mq_det_amd.evaluation.FlickrRecallEvaluator, csrc/flickr_eval.hip): the two fixtures of
tests/test_flickr_eval_cpu.py with the same exact comparisons, the case with more than 64 detections / ground truths per phrase, and the RCCL
exchange in a one-rank group.  Reads tests/golden only.  No time is asserted (tools/flickr_eval_bench.py measures)."""
import os
import socket
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.dirname(HERE))

import test_flickr_eval_cpu as tf  # noqa: E402
from mq_det_amd.evaluation import FlickrRecallEvaluator  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("name", ["small", "merged"])
def test_fixture_on_device_is_exact(name):
    js, a = tf.load_case(name)
    ev = FlickrRecallEvaluator.from_entities_dir(tf.ENT, js["subset"], merge_boxes=js["merge_boxes"], topk=js["topk"], device=DEV)
    tf.feed_raw(ev, js, a, DEV)
    tf.check_score(ev.summarize(), js)
    assert ev.acc.rows.is_cuda and ev.eval["hits"].is_cuda and ev.eval["positives"].dtype == torch.int64
    hits = ev.eval["hits"].cpu()
    ev = tf.from_fixture_gt(js, DEV)
    ev.update(js["post"])                                                          # the reference's post-processed dicts
    tf.check_score(ev.summarize(), js)
    assert torch.equal(ev.eval["hits"].cpu(), hits)


def test_over_64_detections_and_ground_truths_on_device():
    ev = tf.check_random_case(DEV)
    assert ev.eval["dt_box"].is_cuda


def test_rccl_exchange_in_a_one_rank_group():
    import torch.distributed as dist
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
        js, a = tf.load_case("small")
        ev = tf.from_fixture_gt(js, DEV)
        tf.feed_raw(ev, js, a, DEV)
        ev.acc._fold()
        before = ev.acc.rows.clone()
        ev.synchronize_between_processes(force=True)
        assert ev.acc.rows.is_cuda and torch.equal(ev.acc.rows, before)
        tf.check_score(ev.summarize(), js)
    finally:
        if created:
            dist.destroy_process_group()
