"""Random-shape sweep of the kernel SOURCES (through tests/simt, on CPU) against the plain torch restatement of each operator
(tests/ops_emulation.py): shapes the fixed parity checks do not visit -- single rows, lengths around every tile boundary, strides,
masks that empty whole tiles, key splits with empty splits -- drawn from a seeded generator (reproducible; MQ_SIMT_FULL=1: 5x the
draws).  Shipped kernels and the opt-in ones (MQ_ATTN_RESIDENT, MQ_LN_VARIANT, MQ_OFFSET_CONV_VARIANT) go through the same draws.
The families themselves -- drawing and running, apart -- live in tests/fuzz_cases.py; tests/test_gpu_fuzz.py runs the same draws (and
25 x more behind them) on the device.  tests/golden/fuzz_draws.json pins the inputs: the digests of the families this file had before the split
were recorded from its test bodies as they were then.  With MQ_SIMT_DRAWS > 1 a stream is made of ROUNDS (round r holds the base count of every
operator of the family), so the extra draws are other inputs than the 5 x-in-sequence draws of the earlier bodies.
TEST INFRASTRUCTURE ONLY (see tests/test_simt_kernels_cpu.py)."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import fuzz_cases as fc  # noqa: E402

_CXX = os.environ.get("SIMT_CXX", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not os.path.exists(_CXX), reason=f"{_CXX} not found: the kernel-source emulation cannot be built here")
N_DRAWS = int(os.environ.get("MQ_SIMT_DRAWS", "5" if os.environ.get("MQ_SIMT_FULL", "0") == "1" else "1"))     # multiplier of the draw counts
TOL = fc.TOL
SEED = int(os.environ.get("MQ_SIMT_SEED", "0"))                                # offset of every generator seed: other draws


@pytest.fixture(scope="module")
def ops():
    import simt
    with simt.installed() as o:
        yield o


def _sweep(ops, family, tag="", **opt):
    for k, case in enumerate(fc.cases(family, N_DRAWS, seed=SEED, **opt)):
        case["what"] = f"{family}{tag} draw {k}: {case['what']}"
        fc.run(ops, case)


@pytest.mark.parametrize("variant", ["streaming", "resident+chunked"])
def test_attention_random_shapes(ops, monkeypatch, variant):
    monkeypatch.setenv("MQ_ATTN_RESIDENT", "1" if variant != "streaming" else "0")
    _sweep(ops, "attention", f"[{variant}]")


@pytest.mark.parametrize("variant", ["1", "2"])
def test_layernorm_random_shapes(ops, monkeypatch, variant):
    monkeypatch.setenv("MQ_LN_VARIANT", variant)
    _sweep(ops, "layernorm", f"[v{variant}]")


def test_vlfuse_random_shapes(ops):
    _sweep(ops, "vlfuse")


@pytest.mark.parametrize("variant", ["1", "2"])
def test_conv_and_dcn_random_shapes(ops, monkeypatch, variant):
    monkeypatch.setenv("MQ_OFFSET_CONV_VARIANT", variant)
    _sweep(ops, "conv_dcn", f"[v{variant}]", full=variant == "1")


def test_scoring_and_nms_random_shapes(ops):
    _sweep(ops, "scoring_nms")


def test_sparse_attention_and_window_attention_random_shapes(ops):
    _sweep(ops, "sparse_window")


def test_round3_fused_operators_random_shapes(ops):
    """mq_window_attn_qkv_fwd (both widths: resident and streamed weights; images smaller than a window, several trips of the persistent
    workgroups, idle waves), mq_dyrelu_ln_fwd (1 .. 6 levels of ragged sizes) and mq_swin_mlp2_fwd across the pass / tail split."""
    _sweep(ops, "round3_fused")


def test_round4_operators_random_shapes(ops):
    """mq_attn_text_fwd (caption lengths around every 16-key block and the 160-key variant switch, per-item kv_len, max_kv above / at / absent,
    clamp, D = 32 / 64), mq_patch_embed_fwd (both pixel layouts, widths around multiples of 16 patches, C = 96 / 192), and the
    post-processing kernels (mq_post_select_fwd over one / several slices with scores quantised so that ties straddle every cut,
    mq_post_sort_fwd, mq_post_finalize_fwd) against their torch restatements."""
    _sweep(ops, "round4")


def test_grouped_dyconv_kernels_random_pyramids(ops):
    """mq_conv3x3_nchw32_group_fwd and mq_dyconv_epilogue_group on random pyramids (1 .. 6 levels, level sizes around the 8 x 16 tile and
    the 128-position block edges, levels as slices of one token buffer, B = 1 .. 3): the conv against the per-level kernel (fp32 summation
    order apart) and F.conv2d; the epilogue against the per-level launches (bit for bit) with every branch mix (1 .. 3 direct branches,
    with / without a coarser bilinear one)."""
    _sweep(ops, "grouped_dyconv")


def test_swin_mlp_roi_align_and_msdeform_random_shapes(ops):
    _sweep(ops, "swin_roi_msda")


def test_bf16_twins_random_shapes(ops):
    """the *_bf16 entry points on a few of the same draws (tolerance x 8)"""
    _sweep(ops, "bf16_twins")


# ------------------------------------------------------------------------------------------------ families added with the split
NEW_FAMILIES = ("clamped", "patch_merge", "pyramid_elementwise", "vlfuse_masked", "bert_qkv", "gcp_fused", "align_fused", "dcn_stats_group")


@pytest.mark.parametrize("family", NEW_FAMILIES)
def test_added_family_random_shapes(ops, family):
    _sweep(ops, family)


@pytest.mark.parametrize("family", NEW_FAMILIES)
def test_added_family_under_guard_pages(family):
    """the same draws with every library argument against a guard page (tests/simt/guard.py), in a process of its own: an access past an
    argument ends that process, not the session"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "fuzz_cases.py"), family, "all", "--seed", str(SEED), "--device", "cpu"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"{family}: rc {r.returncode}\n{(r.stdout + r.stderr)[-3000:]}"


def test_precise_mode_attention_beyond_the_chunked_kernels_lds(ops):
    """Finding of the sweep (attention draw 0 in the precise mode: D = 64, Nq = 129, Nk = 513): the fp32 tiles of mq_attn_chunked_fwd need 280 KB
    of LDS at D = 64, its launch fails.  ops.attention_chunked_fits states launch_chunked_c's size expression; attention4 sends the shapes it
    refuses to the streaming kernel.  The draw itself runs through the precise-mode emulation in a process of its own."""
    assert ops.attention_chunked_fits(32) and ops.attention_chunked_fits(64)                       # 16-bit operands: 73 KB / 142 KB
    with fc._selected(ops, {"F32_OPERANDS": 1}):
        assert ops.attention_chunked_fits(32) and not ops.attention_chunked_fits(64)               # fp32 tiles: 150 KB / 280 KB of 160 KB
    case = next(iter(fc.cases("attention", 1, seed=0)))
    assert case["D"] == 64 and case["k"].shape[1] > 256 and case["nsplit"] == 1, "draw 0 is no longer the shape of the finding"
    r = subprocess.run([sys.executable, os.path.join(HERE, "fuzz_cases.py"), "attention", "0", "--device", "cpu", "--dtype", "f32", "--env", "MQ_ATTN_RESIDENT=1"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"rc {r.returncode}\n{(r.stdout + r.stderr)[-3000:]}"


def test_served_asks_the_products_predicates(ops):
    """fuzz_cases.served leaves out what the product's own *_fits predicates refuse, in the operand mode of the run"""
    bert = next(c for c in fc.cases("bert_qkv", 4) if c["xs"].shape[1] > 160)
    gcp9 = next(c for c in fc.cases("gcp_fused", 25) if c["op"] == "gcp_attention" and c["idx"].shape[-1] > 8)
    al = next(c for c in fc.cases("align_fused", 4) if c["tk"].shape[1] == 256 and c["kv_max"] == 0)
    assert fc.served(ops, bert) and fc.served(ops, al) and not fc.served(ops, gcp9)
    with fc._selected(ops, {"F32_OPERANDS": 1}):
        assert not fc.served(ops, bert) and not fc.served(ops, al) and not fc.served(ops, gcp9)


# ------------------------------------------------------------------------------------------------ the draws themselves
def test_draws_are_the_inputs_the_sweep_has_always_run():
    """tests/golden/fuzz_draws.json: per family a SHA-256 over the tensors and parameters of its draws at MQ_SIMT_DRAWS=1, MQ_SIMT_SEED=0,
    recorded from the test bodies of this file BEFORE they were split into fuzz_cases.draws / run (every rng / g call in its old order:
    the few that sat between two kernel calls were hoisted).  A rejection by the NMS threshold-margin rule would show here too."""
    with open(os.path.join(HERE, "golden", "fuzz_draws.json")) as f:
        gold = json.load(f)
    assert gold["draws"] == 1 and gold["seed"] == 0
    got = {}
    for key in list(gold["families"]) + list(gold["added_families"]):
        name, _, opt = key.partition("[")
        got[key] = fc.family_digest(name, **fc.parse_opt([opt.rstrip("]")] if opt else []))
    assert set(fc.FAMILIES) == {k.partition("[")[0] for k in got}, "a family without a pinned digest"
    bad = [k for k, v in {**gold["families"], **gold["added_families"]}.items() if got[k] != v]
    assert not bad, f"the draws of {bad} are no longer the recorded ones"


def test_draw_k_does_not_depend_on_the_number_of_rounds():
    """the device's draws (25 x the rounds) START with the emulator's: a stream is made of rounds, draw k is the same case for every n"""
    import hashlib
    for name in ("scoring_nms", "round4"):
        one = list(fc.cases(name, 1))
        three = list(fc.cases(name, 3))
        assert len(three) > 2 * len(one)
        for a, b in zip(one, three):
            ha, hb = hashlib.sha256(), hashlib.sha256()
            fc.case_digest(ha, a)
            fc.case_digest(hb, b)
            assert a["what"] == b["what"] and ha.digest() == hb.digest()


def test_nms_threshold_margin_rule_rejects_few_draws():
    """Exact-match NMS needs well-separated inputs: the generator drops a case in which the float64 IoU of a same-label pair of valid boxes
    lies within 1e-6 of the threshold (inputs alone, the same on CPU and device).  Over the device's draw count it may drop at most 2 %."""
    n = 25
    kept = sum(1 for c in fc.cases("scoring_nms", n) if c["op"] == "ml_nms")
    st = dict(fc.NMS_STATS)
    assert st["drawn"] == 4 * n and kept == st["drawn"] - st.get("rejected", 0)
    assert st.get("rejected", 0) <= 0.02 * st["drawn"], st
    # and the rule itself: a pair moved ONTO the threshold is seen (10 x 10 boxes, "+ 1" convention: IoU = 66 / 176 = 0.375)
    import torch
    boxes = torch.tensor([[[0.0, 0.0, 10.0, 10.0], [5.0, 0.0, 15.0, 10.0], [100.0, 100.0, 110.0, 110.0]]])
    lab, nv = torch.tensor([[1, 1, 1]], dtype=torch.int32), torch.tensor([3], dtype=torch.int32)
    assert fc.nms_margin(boxes, lab, nv, thresh=0.375) <= fc.NMS_MARGIN < fc.nms_margin(boxes, lab, nv, thresh=0.6)
    assert fc.nms_margin(boxes, torch.tensor([[1, 2, 1]], dtype=torch.int32), nv, thresh=0.375) > 0.3        # other label: not a pair
    assert fc.nms_margin(boxes, lab, torch.tensor([1], dtype=torch.int32), thresh=0.375) == float("inf")     # beyond nvalid: never compared


def test_swin_split_draws_follow_the_chip():
    """The Swin-MLP split draws sit around one and two full passes of the machine they run on (dispatch_swin_mlp2's slots): the 4-CU table of the
    emulator, 256 CUs x {4 x 64, 3 x 64, 1 x 128} tokens on the MI355X (check_swin_mlp: C = 384 -> 256 workgroups of 128 tokens, C = 192 -> 768 slots)."""
    assert [fc.swin_slot_tokens(C, fc.EMU_CHIP) for C in (96, 192, 384)] == [16 * 64, 12 * 64, 4 * 128]
    big = {"cus": 256, "f32": False}
    assert [fc.swin_slot_tokens(C, big) for C in (96, 192, 384)] == [1024 * 64, 768 * 64, 256 * 128]
    import torch
    g = torch.Generator().manual_seed(1)
    import random
    seen = 0
    for c in fc.draws_round3_fused(random.Random(1), g, 3, {"cus": 64, "f32": False}):
        if c["op"] == "swin_mlp2":
            C, M = c["x"].shape[1], c["x"].shape[0]
            slot = fc.swin_slot_tokens(C, {"cus": 64, "f32": False})
            assert min(abs(M - slot), abs(M - 2 * slot)) <= 70 or (c["flags"] & 4 and M == fc.SWIN_TAIL_ONLY_MAX_M), (C, M)
            seen += 1
    assert seen == 12
