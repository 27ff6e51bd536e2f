"""TEST INFRASTRUCTURE ONLY.  `python tests/vlfuse_tail.py <cpu|cuda> <guard|nan> <cpu|gpu> [OUT.pt]`: the VLFuse text side
(ops.vlfuse_t2i) with v_ln at the very END of its memory -- against a PROT_NONE page (guard, CPU emulation only) or as the head of a
buffer whose next >= 64 KiB are NaN -- on ragged image-token counts N (the last key tile of an image runs past it), against a float64
softmax(clamp(q k^T)) v written here.  A kernel that reads rows past the last image dies (guard) or returns NaN (0 x NaN in the PV
product); rows of the next image read in place of zeros would not show, the last image's rows past the end do.  Prints `OK <row>` /
`MISMATCH <row> ...` per call and exits 1 on any mismatch; OUT.pt (optional) receives every output for a bit comparison between the
LDS-DMA and the register-ring staging (environment MQ_VL_T2I_DMA, read once per process)."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
HALO_ELEMS = (64 << 10) // 2 + 256            # NaN elements behind v_ln: > 64 KiB

# (B, N, heads, nsplit, masked): N = 1, 63, 65, 70, 130, 1000 on the emulator (every ragged last tile: 1, 63, 1, 6, 2, 40 rows);
# on the device also the token counts of real pyramids -- 18 134 (MQ-GLIP, 800 x 1066), 22 323 (MQ-GroundingDINO, 800 x 1333) and the
# MQ-GLIP benchmark's 22 400 (a multiple of 64)
def cases(which):
    out = []
    if which == "cpu":
        i = 0
        for N in (1, 63, 65, 70, 130, 1000):
            for B in (1, 3):
                for heads in (4, 8):
                    for masked in (False, True):
                        out.append((B, N, heads, 1 + i % 3, masked))
                        i += 1
        return out
    for N, ns in ((1, 3), (63, 2), (65, 3), (18134, 6), (22323, 8), (22400, 6)):
        for B in (1, 3):
            for heads in (4, 8):
                for masked in (False, True):
                    out.append((B, N, heads, ns, masked))
    out += [(16, 22323, heads, 8, masked) for heads in (4, 8) for masked in (False, True)]
    return out


def reference(kf, v, key_mask, clamp):
    """float64: out[b, t, h*256 + c] = sum_n softmax_n(clamp(kf[b, h, t] . v[b, n])) v[b, n, c], masked keys excluded"""
    B, Hh, T, C = kf.shape
    out = torch.empty(B, T, Hh * C, dtype=torch.float64, device=kf.device)
    for b in range(B):
        q, k = kf[b].double(), v[b].double()
        s = torch.einsum("htc,nc->htn", q, k).clamp(-clamp, clamp)
        if key_mask is not None:
            s = s.masked_fill(key_mask[b], float("-inf"))
        out[b] = torch.einsum("htn,nc->thc", s.softmax(-1), k).reshape(T, Hh * C)
    return out


def v_at_the_end(v, follow):
    """a copy of v whose last byte is the last byte before a guard page, or followed by HALO_ELEMS NaN elements"""
    if follow == "guard":
        from simt import guard
        return guard.guarded(v, "end")
    buf = torch.full((v.numel() + HALO_ELEMS,), float("nan"), dtype=v.dtype, device=v.device)
    head = buf[:v.numel()].view(v.shape)
    head.copy_(v)
    return head


def run(dev, follow, which, dtype=torch.float16, out_file=None):
    import parity_checks as pc
    from mq_det_amd import ops
    g = torch.Generator().manual_seed(61)
    T, clamp, bad, outs = (20 if which == "cpu" else 256), 50000.0, 0, {}
    for B, N, heads, ns, masked in cases(which):
        kf = (torch.randn(B, heads, T, 256, generator=g) / 8).to(dtype)
        v = torch.randn(B, N, 256, generator=g).to(dtype)
        mask = None
        if masked:                                            # random padding, every image keeps its first token; the padded last tile too
            mask = torch.rand(B, N, generator=g) < 0.3
            mask[:, 0] = False
            mask[:, N - N // 4:] = True
        kf_d, v_d = kf.to(dev), v_at_the_end(v.to(dev), follow)
        km = None if mask is None else ops.image_key_mask(mask.to(dev))
        got = ops.vlfuse_t2i(kf_d, v_d, ns, clamp=clamp, key_mask=km)
        if dev.type == "cuda":
            torch.cuda.synchronize()
        ref = reference(kf_d, v.to(dev), None if mask is None else mask.to(dev), clamp)
        name = f"vlfuse text side, v_ln at the end ({follow}) B={B} N={N} heads={heads} nsplit={ns} key_mask={masked}"
        r = pc._stat(name, got, ref, tol=pc.TOL)
        finite = bool(torch.isfinite(got).all())
        ok = r["ok"] and finite
        bad += not ok
        print(("OK " if ok else "MISMATCH ") + name + ("" if ok else f" max_err={r['max_err']:.3e} norm={r['norm_err']:.3e} finite={finite}"),
              flush=True)
        outs[name.replace(f"({follow}) ", "")] = got.cpu()
    if out_file:
        torch.save(outs, out_file)
    return bad


def main():
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    kind, follow, which = sys.argv[1:4]
    out_file = sys.argv[4] if len(sys.argv) > 4 else None
    if kind == "cpu":
        import simt
        with simt.installed():
            bad = run(torch.device("cpu"), follow, which, out_file=out_file)
    else:
        from mq_det_amd import ops
        ops.load_library()
        bad = run(torch.device("cuda:0"), follow, which, out_file=out_file)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
