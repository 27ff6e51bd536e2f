"""The random-shape sweep of the TEST.SPECIAL_NMS = 'soft-nms' / 'vote' / 'soft-vote' merges ON THE MI355X: the draws of
tests/tta_special_draws.py that tests/test_tta_special_sweep_cpu.py runs through the emulation, and MQ_GPU_TTA_SWEEP_ROUNDS (default 8) rounds
in all, the first being the emulator's -- classes past one wave and past one 256-row trip, images of several 256-row tiles, the workspace
behind a large class, every position of the top-N cut -- with four waves really running at once: the cross-wave reductions (red_s / red_k /
red_r, red_d), the ballot prefix across trips (run, wcnt) and FL[] between barriers have no other device test at these sizes.  Behind the
draws of a mode: the equal scores laid across the wave boundaries (tta_special_draws.run_ties) and the threshold contract of
tta_cut_rank_kernel over three tiles (run_cut_contract).

One test = one mode, run as `python tests/test_gpu_tta_special_sweep.py <mode> ...` in a child process of its own under a time limit (a
fault fails that test, not the session; one child at a time; nothing retries), once plain and once under halo.poisoned_args("nan"): every
library argument between NaN halos, a write into a halo raises at the entry point, a read of one poisons the result.  After every draw,
tta_special_draws.run also asserts the workspace count, finite outputs and that no output row past counts[b] was written.  The body stops at
the FIRST failing draw, prints the line that replays exactly that draw --

    python tests/tta_special_draws.py <mode> <draw> [--seed S] --device cuda|cpu [--halo]

(--device cpu: through the emulation, every argument against a guard page) -- and exits non-zero.  At most 10 % of a mode's draws may be
rejected by the restated reference's own margins (tta_special_draws.check_rejections).

Measured on an MI355X (256 CUs).  `test_special_merge_on_device_matches_the_reference` in the same visit: 2.40 / 2.43 / 2.56 s (call; soft-nms /
vote / soft-vote); that visit ran 3 rounds (24 draws per child, none rejected): 0.7 - 0.8 s the sweep, 2.9 - 3.0 s the child, 0.8 - 1.0 s and
3.0 - 3.3 s between NaN halos.  With the default 8 rounds, per child: draws run / draws rejected / seconds of the sweep itself (drawing and
the numpy reference included) / seconds of the whole child process (interpreter start, imports, library load).  Every draw passed: no
tolerance was touched, no kernel changed.
  plain     soft-nms 62 / 2 (draws 44 and 54: pick_ratio 1.60, 1.50) / 1.6 / 3.8; vote 64 / 0 / 1.5 / 3.7; soft-vote 64 / 0 / 1.5 / 3.6
  NaN halos soft-nms 62 / 2 / 2.0 / 4.0; vote 64 / 0 / 1.8 / 3.9; soft-vote 64 / 0 / 1.9 / 3.9
The equal-score cases and the cut contract behind the draws: under 0.1 s per child."""
import os
import subprocess
import sys
import time

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.dirname(HERE))

import tta_special_draws as sd  # noqa: E402
import tta_special_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
ROUNDS = int(os.environ.get("MQ_GPU_TTA_SWEEP_ROUNDS", "8"))     # rounds per mode: device draws = len(tta_special_draws.PLANS) x this
SEED = int(os.environ.get("MQ_SIMT_SEED", "0"))


def _child(mode, halo=False, timeout=180):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    cmd = [sys.executable, os.path.abspath(__file__), mode, "--rounds", str(ROUNDS), "--seed", str(SEED)] + (["--halo"] if halo else [])
    t0 = time.time()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    out = r.stdout + r.stderr
    assert r.returncode == 0, f"{' '.join(cmd[1:])}: rc {r.returncode}\n{out[-4000:]}"
    assert "sweep ok" in out, out[-2000:]
    print(out[-400:] + f"child: {time.time() - t0:.1f} s")


@pytest.mark.parametrize("mode", ref.MODES)
def test_special_sweep_on_device(mode):
    _child(mode)


@pytest.mark.parametrize("mode", ref.MODES)
def test_special_sweep_on_device_between_nan_halos(mode):
    _child(mode, halo=True)


def _body(argv):
    """the child: every accepted draw of `rounds` rounds of one mode on the device; the first failing draw ends it"""
    import argparse
    import contextlib
    import traceback
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=ref.MODES)
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--halo", action="store_true")
    a = ap.parse_args(argv)
    from mq_det_amd import ops
    ops.load_library()
    ops.configure()
    dev = torch.device("cuda:0")
    fence = contextlib.nullcontext()
    if a.halo:
        from halo import poisoned_args
        fence = poisoned_args("nan")
    t0, ran = time.time(), 0
    with fence:
        for case in sd.cases(a.mode, a.rounds, a.seed):
            if case["rejected"] is not None:
                print(f"not run: {case['what']}: {case['rejected']}", flush=True)
                continue
            try:
                sd.run(case, dev)
                ran += 1
            except Exception:                                    # noqa: BLE001 -- any failure of a draw: report the replay line, stop
                traceback.print_exc()
                print(f"FAILED {case['what']}" + (" [between NaN halos]" if a.halo else ""))
                for device in ("cuda", "cpu"):
                    print("replay: " + sd.replay_line(a.mode, case["k"], a.seed, device, a.halo), flush=True)
                return 1
        t1 = time.time()
        sd.run_ties(a.mode, dev)
        sd.run_cut_contract(dev)
        torch.cuda.synchronize()
    sd.check_rejections(a.mode)
    st = sd.STATS[a.mode]
    print(f"sweep ok: {a.mode} halo={a.halo}: {ran} draws run, {st['rejected']} rejected, {t1 - t0:.1f} s; ties and cut contract {time.time() - t1:.1f} s",
          flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(_body(sys.argv[1:]))
