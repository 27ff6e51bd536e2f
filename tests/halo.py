"""TEST INFRASTRUCTURE ONLY.  Poison halos around every library argument, on any device (the GPU, or CPU tensors through the kernel-source
emulation of tests/simt).

`poisoned_args(fill)` follows tests/simt/guard.py's pointer_guard: every tensor handed to the library through mq_det_amd.ops._ptr is replaced,
for the duration of the call, by a copy of its WHOLE storage placed in the middle of a fresh buffer on the same device, with HALO bytes on
each side (views keep their offset inside the copy; the copy keeps the original address modulo 256, so no alignment-dependent path of a
kernel changes).  The halos hold

  floating-point arguments: fill "nan" (every byte 0xFF: a NaN in fp32 / fp16 / bf16) or "big" (+65504 in the argument's dtype -- NaN is
                            dropped by fmaxf and v_med3, a large finite value is not: it moves a running max and overflows a dot product);
  integer / bool arguments: zero bytes (the harness never plants a value that a kernel could turn into an address).

A kernel that READS past an argument then takes the poison into its result (the parity check that drives it fails); at ops._chk, after a
device synchronise, both halos of every argument must still hold the fill -- a kernel that WROTE past an argument raises an AssertionError
naming the entry point, the argument, the side and the first changed byte -- and the copies are written back to the original storages.
Calls made while a graph is being captured are passed through unchanged (the pointers would outlive the copies)."""
import contextlib
import ctypes
import sys

import torch

HALO = 64 << 10          # bytes on each side: more than the furthest over-read known (63 rows x 512 B of a VLFuse key tile)
_ALIGN = 256


def _fill_element(dtype, fill):
    """one element of the halo pattern, as bytes"""
    es = torch.empty(0, dtype=dtype).element_size()
    if not dtype.is_floating_point:
        return torch.zeros(es, dtype=torch.uint8)
    if fill == "nan":
        return torch.full((es,), 0xFF, dtype=torch.uint8)
    if fill == "big":
        return torch.tensor([65504.0], dtype=dtype).view(torch.uint8)
    raise ValueError(f"fill must be 'nan' or 'big', not {fill!r}")


def _capturing():
    try:
        return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
    except RuntimeError:
        return False


class _Copy:
    """one storage in the middle of a poisoned buffer"""

    def __init__(self, t, fill, arg):
        st = t.untyped_storage()
        self.key, self.nbytes, self.arg = st.data_ptr(), st.nbytes(), arg
        self.orig = torch.empty(0, dtype=torch.uint8, device=t.device).set_(st)
        el = _fill_element(t.dtype, fill)
        total = HALO + _ALIGN + self.nbytes + HALO
        total = -(-total // el.numel()) * el.numel()
        self.buf = torch.empty(total, dtype=torch.uint8, device=t.device)
        # middle at the original address modulo 256 (the buffer and the storage are both element-aligned: the pattern's phase matches)
        self.off = HALO + (self.key - self.buf.data_ptr() - HALO) % _ALIGN
        self.pattern = el.to(t.device).repeat(total // el.numel())
        self.buf.copy_(self.pattern)
        self.buf[self.off:self.off + self.nbytes].copy_(self.orig)

    def ptr(self, t):
        return self.buf.data_ptr() + self.off + (t.data_ptr() - self.key)

    def check(self, name):
        end = self.off + self.nbytes
        for side, got, want in (("start", self.buf[:self.off], self.pattern[:self.off]), ("end", self.buf[end:], self.pattern[end:])):
            diff = (got != want).nonzero()
            if diff.numel():
                # the changed byte nearest to the argument's storage
                pos = (f"{self.off - int(diff[-1])} bytes before its first byte" if side == "start" else
                       f"{int(diff[0]) + 1} bytes after its last byte")
                raise AssertionError(f"{name}: argument {self.arg}: the {side} halo was written ({pos}, {int(diff.numel())} bytes changed)")

    def restore(self):
        self.orig.copy_(self.buf[self.off:self.off + self.nbytes])


def _arg_name(t, frame, index):
    """the wrapper's local name for t, where it has one (else the argument's position among the call's pointers)"""
    names = [k for k, v in frame.f_locals.items() if v is t] if frame is not None else []
    desc = f"{str(t.dtype).replace('torch.', '')}{list(t.shape)}"
    where = frame.f_code.co_name if frame is not None else "?"
    return f"'{names[0]}' {desc} (ops.{where})" if names else f"#{index} {desc} (ops.{where})"


@contextlib.contextmanager
def poisoned_args(fill="nan"):
    """Inside: every library argument sits between two HALO-byte poison halos (see the module docstring); a write into a halo raises at
    ops._chk, a read of one poisons the result."""
    from mq_det_amd import ops
    live, order = {}, []                                  # storage data_ptr -> _Copy
    real_ptr, real_chk = ops._ptr, ops._chk

    def _ptr(t):
        if t is None or _capturing():
            return real_ptr(t)
        key = t.untyped_storage().data_ptr()
        if key not in live:
            live[key] = _Copy(t, fill, _arg_name(t, sys._getframe(1), len(order)))
            order.append(key)
        return ctypes.c_void_p(live[key].ptr(t))

    def _chk(rc, name):
        if live:
            if any(c.buf.is_cuda for c in live.values()):
                torch.cuda.synchronize()
            copies = [live[k] for k in order]
            live.clear()
            order.clear()
            for c in copies:
                c.restore()
            if rc == 0:                                   # (a failed launch is reported as such by the real _chk)
                for c in copies:
                    c.check(name)
        return real_chk(rc, name)

    ops._ptr, ops._chk = _ptr, _chk
    try:
        yield
    finally:
        ops._ptr, ops._chk = real_ptr, real_chk
