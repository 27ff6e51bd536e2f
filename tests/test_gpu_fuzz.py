"""The random-shape sweep of tests/fuzz_cases.py ON THE MI355X: the draws the emulator sweep runs (tests/test_simt_fuzz_cpu.py) and
MQ_GPU_FUZZ_DRAWS (default 25) times as many behind them, against the same tests/ops_emulation.py restatements at the same stated
tolerances -- real MFMA lane layouts, LDS ordering between waves, LDS-DMA staging, hardware exp / rcp, real atomics and the 256-CU
persistent schedules see shapes they were not tuned on.

One test = one family in one configuration, run as `python tests/test_gpu_fuzz.py <family> ...` in a child process of its own under a
time limit (a fault fails that test, not the session; one child at a time; nothing retries).  The environment selectors are set before
ops.configure() in the child.  The body stops at the FIRST failing draw, prints the line that replays exactly that draw --

    python tests/fuzz_cases.py <family> <draw> --device cuda|cpu --dtype ... [--env ...] [--opt ...]

(--device cpu: through the emulation, every argument against a guard page) -- and exits non-zero.

Configurations:
  fp16        every family; once per kernel selection the operator wrappers read (ops.KERNEL_DEFAULTS): MQ_ATTN_RESIDENT 0 / 1, MQ_LN_VARIANT 1 / 2,
              MQ_OFFSET_CONV_VARIANT 1 / 2 / 3 (with MQ_DCN_BDMA 1 / 0), MQ_VLFUSE_I2T_VARIANT 0 / 1 with MQ_VL_T2I_DMA 1 / 0; MQ_NMS_EARLY_STOP 0 / 1 inside
              every NMS draw.  NOT parametrised: MQ_SWIN_MLP_VARIANT, MQ_DYCONV_EPILOGUE_GROUPED, MQ_PATCH_MERGE_FUSED and MQ_ALIGN_FUSED.  Only
              modeling/pipeline.py reads them, to choose between two OPERATORS; no wrapper in ops does, so setting them would change nothing in these
              bodies.  The operators on either side of each are families instead: swin_mlp2 (round3_fused, swin_roi_msda); dyconv_epilogue_group
              against the per-level launches (grouped_dyconv); patch_merge_ln (patch_merge); align_scores (scoring_nms) and align_fused.  The
              grouped_dyconv family (the group kernel behind MQ_OFFSET_CONV_VARIANT=3) runs under the default selection only.
  bf16        inputs rounded to bf16, tolerance x 8 (the rule of parity_checks.use_dtype)
  f32         MQ_F32_OPERANDS=1, the families behind the test_f32_block names: tolerance min(stated, parity_checks.F32_TOL); draws the precise
              mode does not serve are left out by the product's own predicates (fuzz_cases.served)
  fp16 + NaN  every fp16 family again under halo.poisoned_args("nan"): random shapes between NaN halos

Draw counts: the family's base count (fuzz_cases.FAMILIES[...].base) x MQ_GPU_FUZZ_DRAWS rounds (25; ROUNDS: fewer for a family that takes longer than
`test_block[check_swin_mlp]` in the same visit, never below MIN_MULT, same shape bounds).

Measured on an MI355X (256 CUs), `test_block[check_swin_mlp]` in the same visit: 5.98 s (call).  Per child: draws run / seconds of the sweep itself /
seconds of the whole child process (interpreter start, imports, library load).  Every draw passed in every configuration: no device tolerance was
touched, no kernel changed.
  fp16      attention-ATTN_RESIDENT=0 350 / 0.8 / 2.9; attention-ATTN_RESIDENT=1 350 / 0.8 / 3.0; layernorm-LN_VARIANT=1 400 / 0.9 / 3.0; layernorm-
            LN_VARIANT=2 400 / 1.0 / 3.8; vlfuse-I2T=0-VL_T2I_DMA=1 150 / 1.0 / 3.4; vlfuse-I2T=1-VL_T2I_DMA=0 150 / 1.1 / 3.5; vlfuse_masked-
            VL_T2I_DMA=1 100 / 0.6 / 3.3; vlfuse_masked-VL_T2I_DMA=0 100 / 0.8 / 3.5; conv_dcn-DCN_BDMA=1-OCV=1 125 / 1.0 / 3.7; conv_dcn-OCV=2 125 /
            0.3 / 2.7; conv_dcn-DCN_BDMA=0-OCV=3 125 / 0.8 / 3.0; scoring_nms 300 / 1.7 / 4.2; sparse_window 225 / 0.6 / 2.9; round3_fused 400 / 32.2
            / 34.6 (25 rounds); round4 475 / 2.2 / 4.4; grouped_dyconv 150 / 0.9 / 3.1; swin_roi_msda 275 / 1.6 / 3.9; bf16_twins 500 / 0.7 / 3.0; clamped 300 /
            0.2 / 2.4; patch_merge 150 / 0.2 / 2.4; pyramid_elementwise 400 / 0.6 / 2.9; bert_qkv 75 / 1.6 / 4.0; gcp_fused 94 (+6 not served) / 0.7 /
            2.9; align_fused 100 / 0.4 / 2.7; dcn_stats_group 100 / 1.5 / 3.7
  bf16      attention 350 / 0.8 / 3.0; layernorm 400 / 1.4 / 3.6; vlfuse 150 / 1.1 / 3.2; conv_dcn 125 / 0.9 / 3.0; scoring_nms 300 / 1.6 / 3.9;
            sparse_window 225 / 0.6 / 2.9; round3_fused 160 / 13.3 / 15.6; round4 475 / 2.3 / 4.9; grouped_dyconv 150 / 0.8 / 3.2; swin_roi_msda 275 /
            1.3 / 3.6; clamped 300 / 0.3 / 2.7; patch_merge 150 / 0.2 / 2.4; pyramid_elementwise 400 / 0.6 / 2.9; vlfuse_masked 100 / 0.6 / 2.9;
            bert_qkv 75 / 1.5 / 3.6; gcp_fused 94 (+6 not served) / 0.7 / 3.1; align_fused 100 / 0.4 / 2.6; dcn_stats_group 100 / 1.4 / 3.8
  f32       attention 350 / 1.1 / 3.2; layernorm 400 / 1.4 / 3.5; vlfuse 150 / 1.2 / 3.4; conv_dcn 125 / 0.9 / 3.1; sparse_window 225 / 0.6 / 2.8;
            round3_fused 160 / 3.7 / 5.8; round4 365 (+110 not served) / 2.3 / 4.4; grouped_dyconv 75 (+75 not served) / 0.8 / 2.9; swin_roi_msda 275
            / 2.2 / 4.5; clamped 300 / 0.3 / 2.5; patch_merge 150 / 0.2 / 2.5; vlfuse_masked 100 / 0.9 / 3.4; bert_qkv 46 (+29 not served) / 1.4 /
            3.7; gcp_fused 94 (+6 not served) / 0.8 / 3.0; align_fused 75 (+25 not served) / 0.4 / 2.7; dcn_stats_group 100 / 1.7 / 3.9
  fp16+NaN  attention 350 / 1.2 / 3.5; layernorm 400 / 1.1 / 3.4; vlfuse 150 / 1.6 / 3.8; conv_dcn 125 / 1.0 / 3.2; scoring_nms 300 / 2.7 / 5.0;
            sparse_window 225 / 0.8 / 3.1; round3_fused 160 / 12.3 / 14.7; round4 475 / 3.1 / 5.7; grouped_dyconv 150 / 1.9 / 4.4; swin_roi_msda 275 /
            2.1 / 4.6; bf16_twins 500 / 1.2 / 3.6; clamped 300 / 0.7 / 3.5; patch_merge 150 / 0.3 / 2.8; pyramid_elementwise 400 / 1.0 / 3.7;
            vlfuse_masked 100 / 0.7 / 3.1; bert_qkv 75 / 1.6 / 4.3; gcp_fused 94 (+6 not served) / 0.9 / 3.2; align_fused 100 / 0.6 / 2.9;
            dcn_stats_group 100 / 1.7 / 4.3
round3_fused is the one family above check_swin_mlp's time: 25 rounds (400 draws) took 32.2 s (34.6 s the child) with fp16 operands -- its Swin-MLP
split draws place M around one and two full passes of 256 CUs (up to 2 x 65536 tokens), and the time is the CPU restatement's.  ROUNDS gives it
MIN_MULT = 10 rounds (160 draws): 15.4 s the fp16 child, bf16 / f32 / NaN halos as above.  It stays above 5.98 s at that floor; the shape bounds are not lowered."""
import os
import subprocess
import sys
import time

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.dirname(HERE))

import fuzz_cases as fc  # noqa: E402

pytestmark = pytest.mark.gpu
MULT = int(os.environ.get("MQ_GPU_FUZZ_DRAWS", "25"))            # rounds per family: device draws = the family's base count x this
MIN_MULT = 10
# families whose 25 rounds took longer than test_block[check_swin_mlp] on the same visit run fewer rounds (never below MIN_MULT; same shape bounds)
ROUNDS = {"round3_fused": 10}
SEED = int(os.environ.get("MQ_SIMT_SEED", "0"))

# (family, env, draw options): the kernel selections of the fp16 runs
SELECTIONS = [
    ("attention", {"MQ_ATTN_RESIDENT": "0"}, {}), ("attention", {"MQ_ATTN_RESIDENT": "1"}, {}),
    ("layernorm", {"MQ_LN_VARIANT": "1"}, {}), ("layernorm", {"MQ_LN_VARIANT": "2"}, {}),
    ("vlfuse", {"MQ_VLFUSE_I2T_VARIANT": "0", "MQ_VL_T2I_DMA": "1"}, {}), ("vlfuse", {"MQ_VLFUSE_I2T_VARIANT": "1", "MQ_VL_T2I_DMA": "0"}, {}),
    ("vlfuse_masked", {"MQ_VL_T2I_DMA": "1"}, {}), ("vlfuse_masked", {"MQ_VL_T2I_DMA": "0"}, {}),
    ("conv_dcn", {"MQ_OFFSET_CONV_VARIANT": "1", "MQ_DCN_BDMA": "1"}, {"full": "1"}), ("conv_dcn", {"MQ_OFFSET_CONV_VARIANT": "2"}, {"full": "0"}),
    ("conv_dcn", {"MQ_OFFSET_CONV_VARIANT": "3", "MQ_DCN_BDMA": "0"}, {"full": "1"}),
]
_SELECTED = {s[0] for s in SELECTIONS}
FP16 = SELECTIONS + [(name, {}, {}) for name in fc.FAMILIES if name not in _SELECTED]
# the default selection of every family, for the other operand modes (the precise mode has no second VLFuse image-side variant: ops.vlfuse_i2t
# takes variant 0 there whatever is selected; the grouped offset conv is refused by conv3x3_nchw32_group_supported, which fuzz_cases.served asks)
DEFAULTS = [(name, {}, {}) for name in fc.FAMILIES]


def _id(cfg):
    name, env, opt = cfg
    return name + "".join(f"-{k[3:]}={v}" for k, v in sorted(env.items()))


def _rounds(name):
    return max(MIN_MULT, min(MULT, ROUNDS.get(name, MULT))) if MULT >= MIN_MULT else MULT


def _child(cfg, dtype, halo=False, timeout=420):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    name, env, opt = cfg
    cmd = [sys.executable, os.path.abspath(__file__), name, "--dtype", dtype, "--rounds", str(_rounds(name)), "--seed", str(SEED)]
    if env:
        cmd += ["--env"] + [f"{k}={v}" for k, v in sorted(env.items())]
    if opt:
        cmd += ["--opt"] + [f"{k}={v}" for k, v in sorted(opt.items())]
    if halo:
        cmd.append("--halo")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    out = r.stdout + r.stderr
    assert r.returncode == 0, f"{' '.join(cmd[1:])}: rc {r.returncode}\n{out[-4000:]}"
    print(out[-300:])


@pytest.mark.parametrize("cfg", FP16, ids=_id)
def test_fp16(cfg):
    _child(cfg, "fp16")


@pytest.mark.parametrize("cfg", [c for c in DEFAULTS if fc.FAMILIES[c[0]].bf16], ids=_id)
def test_bf16(cfg):
    _child(cfg, "bf16")


@pytest.mark.parametrize("cfg", [c for c in DEFAULTS if fc.FAMILIES[c[0]].f32], ids=_id)
def test_f32_operands(cfg):
    _child(cfg, "f32")


@pytest.mark.parametrize("cfg", DEFAULTS, ids=_id)
def test_fp16_between_nan_halos(cfg):
    _child(cfg, "fp16", halo=True)


def _body(argv):
    """the child: every draw of `rounds` rounds of one family on the device; the first failing draw ends it"""
    import argparse
    import contextlib
    import traceback
    ap = argparse.ArgumentParser()
    ap.add_argument("family", choices=sorted(fc.FAMILIES))
    ap.add_argument("--dtype", choices=("fp16", "bf16", "f32"), default="fp16")
    ap.add_argument("--rounds", type=int, default=MULT)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--env", nargs="*", default=[])
    ap.add_argument("--opt", nargs="*", default=[])
    ap.add_argument("--halo", action="store_true")
    a = ap.parse_args(argv)
    env = dict(kv.split("=", 1) for kv in a.env)
    os.environ.update(env)                                       # before ops.configure(): the selection is read once
    if a.dtype == "f32":
        os.environ["MQ_F32_OPERANDS"] = "1"
    from mq_det_amd import ops
    ops.load_library()
    ops.configure()
    dev = torch.device("cuda:0")
    chip = fc.device_chip(a.dtype == "f32")
    opt = dict(kv.split("=", 1) for kv in a.opt)
    fence = contextlib.nullcontext()
    if a.halo:
        from halo import poisoned_args
        fence = poisoned_args("nan")
    t0, skipped, k = time.time(), 0, -1
    with fence:
        for k, case in enumerate(fc.cases(a.family, a.rounds, chip, a.seed, **fc.parse_opt(a.opt))):
            case = fc.cast_case(case, a.dtype)
            case["what"] = f"{a.family} draw {k}: {case['what']}"
            if not fc.served(ops, case):
                skipped += 1
                continue
            try:
                fc.run(ops, case, lambda t: t.to(dev))
                torch.cuda.synchronize()
            except Exception:                                    # noqa: BLE001 -- any failure of a draw: report the replay line, stop
                traceback.print_exc()
                print(f"FAILED {case['what']}" + (" [between NaN halos]" if a.halo else ""))
                for device in ("cuda", "cpu"):
                    line = fc.replay_line(a.family, k, a.seed, device, a.dtype, env, opt)
                    print("replay: " + line + (f" --cus {chip['cus']}" if device == "cpu" else ""), flush=True)
                return 1
    if a.family == "scoring_nms":
        st = fc.NMS_STATS
        assert st.get("rejected", 0) <= 0.02 * st["drawn"], f"the NMS threshold-margin rule rejected {st}"
    print(f"fuzz ok: {a.family} dtype={a.dtype} env={env} halo={a.halo}: {k + 1 - skipped} draws run, {skipped} not served, {time.time() - t0:.1f} s", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(_body(sys.argv[1:]))
