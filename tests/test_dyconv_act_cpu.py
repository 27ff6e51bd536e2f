"""mq_dyconv_coef_relu_group and mq_dyconv_fuse_act_group (KERNELS["DYCONV_EPILOGUE_LN"]) through the kernel-source emulation of tests/simt:
the checks of tests/dyconv_act_checks.py on CPU tensors -- branch coefficients bit-equal to mq_dyconv_coef_group, DYReLU coefficients from the
DCN statistics against a float64 restatement (no worse than the pooled ones), the fused pass bit-equal to fuse + mq_dyrelu_ln_fwd (mode LN) and
to fuse + mq_dyrelu_apply (mode ReLU) -- fp16 and bf16, under permuted thread schedules, and against guard pages in a process of their own.
The same checks on the device: tests/test_gpu_dyconv_act.py."""
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

CPU = torch.device("cpu")
_CXX = os.environ.get("SIMT_CXX", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not os.path.exists(_CXX), reason=f"{_CXX} not found: the kernel-source emulation cannot be built here")


@pytest.fixture(scope="module")
def emu():
    import simt
    with simt.installed():
        yield simt


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", range(4))
def test_kernels(emu, case, dtype):
    import dyconv_act_checks as dc
    B, sizes = dc.PYRAMIDS[case]
    dc.run_case(B, sizes, dtype, CPU, seed=40 + case)


@pytest.mark.parametrize("schedule", [("descending", 0), ("random", 5)], ids=lambda s: s[0])
def test_kernels_under_permuted_schedules(emu, schedule):
    """the LDS operands of the fused pass and the shared reduction arrays of the coefficient kernel are published by barriers, not by thread order"""
    import dyconv_act_checks as dc
    emu.set_schedule(*schedule)
    try:
        for case in (0, 3):
            B, sizes = dc.PYRAMIDS[case]
            dc.run_case(B, sizes, torch.float16, CPU, seed=40 + case)
    finally:
        emu.set_schedule("ascending")


@pytest.mark.parametrize("mode", ["end", "start"])
def test_kernels_against_guard_pages(mode):
    """every argument of the two entry points (and of the ones they are compared with) against a PROT_NONE page: a read or write outside a
    buffer ends the child with SIGSEGV"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK guarded" in r.stdout, f"rc {r.returncode}\n{(r.stdout + r.stderr)[-2000:]}"


def test_the_plain_torch_stand_in_keeps_the_old_calls():
    """vldyhead takes the new path only with an ops namespace that has both wrappers: the plain-torch stand-in of the CPU pipeline tests
    (tests/ops_emulation.py) carries the switch in its KERNELS table but not the wrappers, so it keeps dyconv_tokens + dyrelu_layer_norm"""
    import ops_emulation
    from mq_det_amd import ops
    fake = ops_emulation.namespace(ops)
    assert "DYCONV_EPILOGUE_LN" in fake.KERNELS
    assert hasattr(ops, "dyconv_coef_relu_group") and hasattr(ops, "dyconv_fuse_act_group")
    assert not hasattr(fake, "dyconv_coef_relu_group") and not hasattr(fake, "dyconv_fuse_act_group")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    import simt
    from simt import guard
    import dyconv_act_checks as dc
    with simt.installed(), guard.pointer_guard(sys.argv[1]), guard.guarded_ops(sys.argv[1]):
        dc.run_all(CPU)
    print("OK guarded", sys.argv[1])
