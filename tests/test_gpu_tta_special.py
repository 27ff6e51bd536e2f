"""TEST.SPECIAL_NMS = 'soft-nms' / 'vote' / 'soft-vote' of the TTA merge on the MI355X: mq_tta_merge_special against the numpy restatement
(tests/tta_special_ref.py) and the recorded reference (tests/golden/tta_special), by the rules of tests/tta_special_cases.py -- the same
cases tests/test_tta_special_cpu.py runs through the kernel sources' emulation.  No model forward; all cases of a mode share one process
(one library load), run under a time limit of its own: a fault or a hang fails that test, not the session."""
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.dirname(HERE))

import tta_special_cases as sc  # noqa: E402
import tta_special_ref as ref  # noqa: E402
from mq_det_amd import tta  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]
DEV = torch.device("cuda:0")


def _body_mode(mode):
    import test_tta_special_cpu as tcs
    dets = sc.to_device(sc.build_dets(), DEV)
    tta._WARNED_CLASSES = True
    for name, th, top_n in sc.CASES[mode]:
        want = sc.expected(mode, th, top_n)
        sc.check_conditions(mode, th, want)
        for cap in (None, sc.FORCED_CAP):
            stats = {}
            got = tta.merge(dets, sc.WH, sc.make_cfg(mode, th, top_n), DEV, row_cap=cap, stats=stats)
            assert all(r.bbox.is_cuda for r in got)
            assert (stats["workspace_classes"] > 0) == (cap is not None and th > 0), (name, cap, stats)
            sc.compare(mode, th, sc.host(got), want, f"{mode} {name} cap {cap}")
            print(f"OK {mode} {name} cap {cap}: {[len(r) for r in got]} rows, {stats['workspace_classes']} classes through the workspace", flush=True)
    js, a = tcs.load_gold()
    for name, th, top_n in sc.CASES[mode]:
        if th <= 0:
            continue
        want = tcs.gold_expected(js, a, f"{mode}_{name}")
        for cap in (None, sc.FORCED_CAP):
            stats = {}
            got = tta.merge_result_from_multi_scales(tcs.gold_boxlists(js, a, DEV), sc.make_cfg(mode, th, top_n), row_cap=cap, stats=stats)
            assert (stats["workspace_classes"] > 0) == (cap is not None)
            sc.compare(mode, th, sc.host(got), want, f"fixture {mode} {name} cap {cap}")
    print(f"OK {mode}: recorded fixture through merge_result_from_multi_scales", flush=True)


def _body_none():
    import test_tta_special_cpu as tcs
    tcs.check_mode_none(DEV)
    print("OK mode 'none' of merge_result_from_multi_scales = tta.merge", flush=True)


def _run(*args, timeout=120):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *args], capture_output=True, text=True, timeout=timeout)
    out = r.stdout + r.stderr
    assert r.returncode == 0, f"{args}: rc {r.returncode}\n{out[-4000:]}"
    return out


@pytest.mark.parametrize("mode", ref.MODES)
def test_special_merge_on_device_matches_the_reference(mode):
    out = _run("mode", mode)
    assert out.count("OK ") == 7, out[-2000:]


def test_mode_none_of_the_public_function_is_the_existing_merge_on_device():
    _run("none")


if __name__ == "__main__":
    if sys.argv[1] == "mode":
        _body_mode(sys.argv[2])
    else:
        _body_none()
