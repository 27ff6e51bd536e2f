"""world-2 gloo worker of tests/test_flickr_eval_cpu.py: FlickrRecallEvaluator's exchange.  Rank r feeds the sentences n with n % 2 == r of the
small fixture; rank 1 also sends sentence 0 again with boxes that hit nothing (rank 0's arrived first: dropped).  Both ranks summarize
through the kernel-source emulation and must get the fixture's score."""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def main():
    import torch.distributed as dist
    sys.path.insert(0, HERE)
    sys.path.insert(1, ROOT)
    import simt
    import test_flickr_eval_cpu as tf
    from mq_det_amd import parallel

    rank, local, world = parallel.init_distributed("gloo")
    assert world == 2
    js, a = tf.load_case("small")
    ev = tf.from_fixture_gt(js)
    n_sent = len(js["sentences"])
    tf.feed_raw(ev, js, a, which={n for n in range(n_sent) if n % 2 == rank})
    if rank == 1:
        s = js["sentences"][0]
        ev.update_boxlist(s["image_id"], s["sentence_id"], tf.boxlist(np.zeros((1, 4), np.float32), np.ones(1, np.float32), np.array([js["plus"]]), s["size"]),
                          s["n_phrases"], js["plus"], s["orig_size"])
    own = len(ev.acc.rows) + sum(len(r) for r in ev.acc._pending)
    ev.synchronize_between_processes()
    assert len(ev.acc.rows) > own
    with simt.installed(), warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        score = ev.summarize()
    tf.check_score(score, js)
    assert ev.eval["flags"].tolist() == [1, 0, 0, 0] and any("multiple predictions" in str(x.message) for x in w)
    dist.barrier()
    print("FLICKR_GATHER_OK", rank, len(ev.acc.rows), flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
