"""One setting of the DCNv2 A/B switches per PROCESS (csrc/dcn_fused.hip reads MQ_DCN_WAVES / _SYNC / _PLAIN / _RASTER once; KERNELS["DCN_BDMA"]
comes from MQ_DCN_BDMA at import): the grouped launch on the smallest shapes that cross every boundary of the kernel, against the torch
restatement of tests/ops_emulation.py.

    python tests/dcn_switches.py cpu|gpu out.pt          (the switches in the environment)

B = 1, C = 128 (one weight slice per tap group: the least the kernel accepts), a 9 x 17 input at stride 1 (153 positions: one full 128-row tile
and a ragged one) and at stride 2 (5 x 9 = 45: one ragged tile) as ONE grouped launch -- once with random offsets and mask logits, once as the
plain convolution (zero offsets, mask 1, flags bit 1: the PLAIN instantiations where the setting has them).  Tolerance: 4e-3 of the range, the
DCNv2 rows of tests/parity_checks.py.  cpu: the lane-by-lane emulation of the kernel source; gpu: the device.  Exit status 1 on a mismatch;
the outputs go to out.pt for the caller (test_simt_kernels_cpu.py, test_gpu_parity.py) to compare settings with."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TOL = 4e-3
SETTINGS = (("default", {}), ("waves8", {"MQ_DCN_WAVES": "8"}), ("sync2_rowmajor", {"MQ_DCN_SYNC": "2", "MQ_DCN_BDMA": "0"}),
            ("plain0", {"MQ_DCN_PLAIN": "0"}), ("rowmajor", {"MQ_DCN_BDMA": "0"}), ("raster0", {"MQ_DCN_RASTER": "0"}))


def run_settings(where, tmp, timeout):
    """The six settings, one child process each, in sequence; stops at the first child that fails.  -> {name: outputs}."""
    import subprocess
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MQ_DCN_")}
    outs = {}
    for name, env in SETTINGS:
        f = os.path.join(tmp, name + ".pt")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), where, f], env=dict(clean, **env), capture_output=True, text=True, timeout=timeout)
        assert r.returncode == 0, f"{name} {env}: exit status {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}"
        outs[name] = torch.load(f)
    return outs


def main(where, out):
    import contextlib
    import ops_emulation as emu
    from mq_det_amd import ops
    dev = torch.device("cuda:0" if where == "gpu" else "cpu")
    g = torch.Generator().manual_seed(23)
    x = torch.randn(1, 9, 17, 128, generator=g).half()
    w = (torch.randn(256, 9 * 128, generator=g) / 34).half()
    bias = torch.randn(256, generator=g).half()
    oms = {1: torch.randn(1, 27, 9, 17, generator=g) * 1.5, 2: torch.randn(1, 27, 5, 9, generator=g) * 1.5}
    groups = {}
    for kind in ("offsets", "plain"):
        brs = []
        for stride in (1, 2):
            om = oms[stride]
            if kind == "plain":                      # pipeline._zero_offsets: sigmoid(100) == 1.0f
                om = torch.cat([torch.zeros_like(om[:, :18]), torch.full_like(om[:, 18:], 100.0)], 1)
            brs.append({"x": x, "om": om.contiguous(), "w": w, "bias": bias, "stride": stride, "plain": kind == "plain"})
        groups[kind] = brs
    if where == "cpu":
        import simt
        ctx = simt.installed()
    else:
        ctx = contextlib.nullcontext()
    got, bad = {}, 0
    with ctx:
        for kind, brs in groups.items():
            ys = ops.dcnv2_group([{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in br.items()} for br in brs], want_stats=False)
            if where == "gpu":
                torch.cuda.synchronize()
            for br, (y, hw, _) in zip(brs, ys):
                ref, hw_ref = emu.dcnv2(br["x"], br["om"], br["w"], br["bias"], br["stride"])
                y = y.cpu()
                err = (y.float() - ref.float()).abs().max().item()
                scale = max(1.0, ref.float().abs().max().item())
                ok = tuple(hw) == tuple(hw_ref) and err == err and err <= TOL * scale
                print(f"{kind} stride {br['stride']}: max err {err:.3e}, range {scale:.3f}, norm {err / scale:.3e} (tol {TOL:.0e}) {'ok' if ok else 'MISMATCH'}")
                bad += not ok
                got[f"{kind}_s{br['stride']}"] = y
    torch.save(got, out)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
