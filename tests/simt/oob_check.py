"""TEST INFRASTRUCTURE ONLY.  `python tests/simt/oob_check.py <mode> <check> [<check> ...]`: run parity checks on the emulated kernels
with every library argument against a guard page (tests/simt/guard.py, mode "end" / "start"), or between two poison halos (tests/halo.py,
mode "halo-nan" / "halo-big"); prints `OK <check>` per check.  A kernel that reads or writes outside one of its buffers on the guarded
side ends this process with SIGSEGV -- the caller (tests/test_simt_kernels_cpu.py) looks at the return code; under the halos a read
shows as a failed parity row and a write as an AssertionError."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def pooled_tokens(dev=None):
    """the body of test_pooled_tokens_fused_equals_avg_pool_and_cat: mq_pool2x2_tokens_fwd == five avg_pool2d + concat, bit for bit"""
    import torch
    import torch.nn.functional as F
    from mq_det_amd import ops
    g = torch.Generator().manual_seed(13)
    res = []
    for dt in (torch.float16, torch.bfloat16):
        for sizes in (((100, 168), (50, 84), (25, 42), (13, 21), (7, 11)), ((9, 7), (5, 4), (3, 2)), ((2, 2),)):
            big = [torch.randn(3, h, w, 256, generator=g).to(dt) for h, w in sizes]
            feats = [x[:2].permute(0, 3, 1, 2) for x in big]
            ref = torch.cat([F.avg_pool2d(f.float(), 2).to(dt).permute(0, 2, 3, 1).flatten(1, 2) for f in feats], 1)
            got = ops.pool2x2_tokens([x.to(dev)[:2].permute(0, 3, 1, 2) for x in big] if dev is not None else feats).cpu()
            res.append({"name": f"pool2x2_tokens {dt} {sizes}", "ok": got.shape == ref.shape and torch.equal(got, ref)})
    return res


def main():
    import contextlib
    import torch
    import simt
    from simt import guard
    import halo
    import parity_checks as pc
    import gdino_checks as gc
    from mq_det_amd.modeling import detector, pipeline
    mode, names = sys.argv[1], sys.argv[2:]
    cpu = torch.device("cpu")

    def prepare(self, device=None):
        self._validate_config()
        self._plan = pipeline.build_plan(self.state_dict(), self.cfg, cpu, dtype=detector.compute_dtype(self.cfg))
        self._plan_key, self.use_hip_graph = cpu, False
        return self._plan
    detector.GeneralizedVLRCNN_New.prepare = prepare
    pc.QUICK, pc.PINS = True, False
    extra = {
        "attention_small": lambda: [pc.check_attention(cpu, B=2, H=3, D=64, Nq=70, Nk=141, mask=True, kvlen=True),
                                    pc.check_attention(cpu, B=1, H=2, D=32, Nq=37, Nk=61),
                                    pc.check_attention(cpu, B=1, H=2, D=32, Nq=37, Nk=700, nsplit=2),
                                    pc.check_attention(cpu, B=1, H=2, D=64, Nq=130, Nk=257, mask=True, clamp=50000.0)],
        "pooled_tokens": pooled_tokens,
    }
    if mode.startswith("halo-"):
        fences = halo.poisoned_args(mode[len("halo-"):])
    else:
        fences = contextlib.ExitStack()
        fences.enter_context(guard.pointer_guard(mode))
        fences.enter_context(guard.guarded_ops(mode))
    with simt.installed(), fences:
        for n in names:
            fn = extra.get(n) or (lambda n=n: getattr(pc, n, None)(cpu) if hasattr(pc, n) else getattr(gc, n)(cpu))
            res = fn()
            res = res if isinstance(res, list) else [res]
            bad = [r["name"] for r in res if not r["ok"] and "HIP-graph" not in r["name"]]
            print(("OK " if not bad else "MISMATCH ") + n + (" " + "; ".join(bad[:3]) if bad else ""), flush=True)


if __name__ == "__main__":
    main()
