"""Out-of-bounds access on the device: what the CPU guard pages (tests/simt/guard.py) see on the emulated kernels, seen on the MI355X.

A read past an argument that lands on finite bytes, or a write past it into memory no check reads, passes every parity check.  Here
every library argument sits between two 64 KiB poison halos (tests/halo.py): NaN or +65504 halos must leave the parity rows at their
gates, and both halos of every argument unchanged.  Then the VLFuse text side with v_ln followed by NaN at real pyramid sizes, and one
whole fusion layer at an image size whose token count is not a multiple of 64.  Every body runs in a process of its own under a time limit
(a wrong address on the device kills the process, not a test)."""
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    from mq_det_amd import ops
    ops.load_library()
    return torch.device("cuda:0")


def _run(args, timeout, env=None):
    r = subprocess.run([sys.executable, *args], capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **(env or {})))
    return r.returncode, r.stdout + r.stderr


# the checks of the CPU guard-page list (tests/test_simt_kernels_cpu.py: OOB_NAMES + OOB_NAMES_FULL), all of which pass the guard pages
# on both sides there
HALO_CHECKS = ["attention_small", "check_layernorm", "check_window_attention", "check_conv3x3", "check_bert_attn_qkv", "check_gcp_attn_fused",
               "check_vlfuse_kernels", "check_vlfuse_heads_mask", "check_dcn", "check_dyconv", "check_swin_fpn", "pooled_tokens",
               "check_gcp_block", "check_pre_select", "check_vl_fuse", "check_post_golden", "check_score_agg", "check_nms", "check_swin_mlp",
               "check_roi_align", "check_msdeform_attn", "check_attention_qk_mask", "check_msdeform_attn_q", "check_attention_strided"]
HALO_CHECKS_BF16 = ["check_vlfuse_kernels", "check_vlfuse_heads_mask", "check_dcn"]


def _body_poisoned(fill, dtype, names):
    import parity_checks as pc
    import gdino_checks as gc
    from halo import poisoned_args
    sys.path.insert(0, os.path.join(HERE, "simt"))
    import oob_check
    dev = torch.device("cuda:0")
    pc.use_dtype(torch.bfloat16 if dtype == "bf16" else torch.float16)
    extra = {"attention_small": lambda: [pc.check_attention(dev, B=2, H=3, D=64, Nq=70, Nk=141, mask=True, kvlen=True),
                                         pc.check_attention(dev, B=1, H=2, D=32, Nq=37, Nk=61),
                                         pc.check_attention(dev, B=1, H=2, D=32, Nq=37, Nk=700, nsplit=2),
                                         pc.check_attention(dev, B=1, H=2, D=64, Nq=130, Nk=257, mask=True, clamp=50000.0)],
             "pooled_tokens": lambda: oob_check.pooled_tokens(dev)}
    bad = 0
    with poisoned_args(fill):
        for n in names:
            fn = extra.get(n) or (lambda n=n: getattr(pc, n)(dev) if hasattr(pc, n) else getattr(gc, n)(dev))
            res = fn()
            res = res if isinstance(res, list) else [res]
            torch.cuda.synchronize()
            rows = [r for r in res if not r["ok"] and "HIP-graph" not in r["name"]]
            bad += bool(rows)
            print(("OK " if not rows else "MISMATCH ") + n + "".join(f"\n  {r['name']}: norm_err {r.get('norm_err', float('nan')):.3e} tol {r.get('tol', 0):.1e}"
                                                                for r in rows[:5]), flush=True)
    return bad


@pytest.mark.parametrize("fill", ["nan", "big"])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_no_kernel_reads_or_writes_the_poison_halos(dev, fill, dtype):
    """every argument of every call between two poison halos: the parity rows pass at their usual gates (a read past an argument would
    bring NaN / 65504 into a result) and every halo is intact at ops._chk (a write past one raises there)"""
    names = HALO_CHECKS if dtype == "fp16" else HALO_CHECKS_BF16
    rc, out = _run([os.path.abspath(__file__), "poisoned", fill, dtype, *names], timeout=1500)
    lines = [ln for ln in out.splitlines() if ln.startswith(("OK ", "MISMATCH "))]
    assert rc == 0 and lines == ["OK " + n for n in names], f"rc {rc}\n{out[-4000:]}"


def test_vlfuse_text_side_reads_nothing_past_the_last_image(dev, tmp_path):
    """tests/vlfuse_tail.py on the device: v_ln as the head of a buffer whose next 64 KiB are NaN; N = 1, 63, 65, 18 134 (MQ-GLIP at
    800 x 1066), 22 323 (MQ-GroundingDINO at 800 x 1333), 22 400; 1, 3 and 16 images; 4 and 8 heads; with and without an image key mask;
    against float64 at TOL with no NaN -- on the LDS-DMA staging and on the register ring, which give the same bits"""
    outs = {}
    for dma in ("1", "0"):
        outs[dma] = str(tmp_path / f"dma{dma}.pt")
        rc, out = _run([os.path.join(HERE, "vlfuse_tail.py"), "cuda", "nan", "gpu", outs[dma]], timeout=900, env={"MQ_VL_T2I_DMA": dma})
        assert rc == 0, f"MQ_VL_T2I_DMA={dma}: rc {rc}\n" + "\n".join(ln for ln in out.splitlines() if not ln.startswith("OK "))[-4000:]
    a, b = torch.load(outs["1"]), torch.load(outs["0"])
    assert a.keys() == b.keys() and len(a) == 52
    diff = [k for k in a if not torch.equal(a[k], b[k])]
    assert not diff, diff[:5]


def _body_fusion_layer_800x1066():
    import parity_checks as pc
    dev = torch.device("cuda:0")
    sizes = ((100, 136), (50, 68), (25, 34), (13, 17), (7, 9))           # 800 x 1066 padded to 800 x 1088: N = 18 134 = 283 x 64 + 22
    assert sum(h * w for h, w in sizes) == 18134
    res = pc.check_fusion_layer(dev, sizes=sizes)
    bad = 0
    for r in res:
        tol = r["tol"]
        # the image-token rows carry the level size in their name: the gate of the same row at the 22 400-token benchmark pyramid
        m = pc._measured(r["name"].replace("@ 100x136", "@ 100x168"))
        if m is not None and pc.MEASURED_GATE:
            tol = min(tol, max(pc.MEASURED_FLOOR, pc.MEASURED_MARGIN_DEEP * m))
        ok = r["ok"] and r["norm_err"] <= tol
        print(("OK " if ok else "MISMATCH ") + f"{r['name']}: norm_err {r['norm_err']:.3e} tol {tol:.2e}", flush=True)
        bad += not ok
    return bad


def test_fusion_layer_at_a_pyramid_that_is_not_a_multiple_of_64(dev):
    """one whole fusion layer (VLFuse both ways, clamped BERT layer, DyConv / DCNv2) at the 800 x 1066 pyramid -- 18 134 tokens, 22 in the
    last key tile -- against the oracle, at the tolerances of the 22 400-token benchmark row"""
    rc, out = _run([os.path.abspath(__file__), "fusion_layer_800x1066"], timeout=900)
    assert rc == 0 and "MISMATCH" not in out, f"rc {rc}\n{out[-4000:]}"


if __name__ == "__main__":                       # python tests/test_gpu_halo.py <body> [args]: one isolated body
    sys.path.insert(0, os.path.dirname(HERE))
    from mq_det_amd import ops as _ops
    _ops.load_library()
    _bad = _body_poisoned(sys.argv[2], sys.argv[3], sys.argv[4:]) if sys.argv[1] == "poisoned" else globals()["_body_" + sys.argv[1]]()
    torch.cuda.synchronize()
    print("body done:", sys.argv[1], "mismatches:", _bad)
    sys.exit(1 if _bad else 0)
