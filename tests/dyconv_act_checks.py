"""Checks of mq_dyconv_coef_relu_group and mq_dyconv_fuse_act_group (csrc/dyconv.hip, KERNELS["DYCONV_EPILOGUE_LN"]), shared by the
emulation run (tests/test_dyconv_act_cpu.py) and the device run (tests/test_gpu_dyconv_act.py); with them mq_dyrelu_apply_group
(KERNELS["DYRELU_APPLY_GROUPED"]): all levels of the buffer in one launch, bit-equal to mq_dyrelu_apply level by level.

Inputs: random DCN outputs y of every branch of a small pyramid with their statistics part[b, blk, c, 0..2] = per-block (sum y, sum y^2,
sum w_p y) restated in torch (8 positions per block, so that a level has 1 .. 60 partials: both loops of the four reducers run), w_p = 1/n
or the bilinear pooling weights of pipeline._upsample_pool_weights.  Branches per level as the head builds them: the level's own map, one
more map at the level's resolution below the top of the pyramid, and the next coarser level's map read through the bilinear sampler."""
import torch
import torch.nn.functional as F

PYRAMIDS = ((2, [(20, 24), (10, 12), (5, 6), (3, 3), (2, 2)]),
            (2, [(17, 9), (9, 5)]),
            (2, [(13, 21)]),                                   # a single level, no bilinear branch
            (3, [(9, 17), (8, 16), (1, 1)]))
FLOOR = 300 * 2.0 ** -24         # fp32 rounding of the FC reductions over 256 and 64 terms
EPS_GN, EPS_LN, GROUPS = 1e-5, 1e-5, 16
ROWS_PER_PART = 8


def _partials(y, w):
    """y [B, n, C] (16-bit), w [n] fp64 -> [B, ceil(n / 8), C, 3] fp32"""
    B, n, C = y.shape
    nblk = -(-n // ROWS_PER_PART)
    y64 = y.double().cpu()
    pad = nblk * ROWS_PER_PART - n
    y64 = F.pad(y64, (0, 0, 0, pad))
    w64 = F.pad(w.double().cpu(), (0, pad))
    yb, wb = y64.reshape(B, nblk, ROWS_PER_PART, C), w64.reshape(1, nblk, ROWS_PER_PART, 1)
    return torch.stack([yb.sum(2), (yb * yb).sum(2), (yb * wb).sum(2)], -1).float().contiguous()


def make_case(B, sizes, dtype, dev, seed):
    """-> dict: per-branch items (y, sums, n, hs, ws, gamma, beta, nbranches, level), attention / DYReLU / LayerNorm weights"""
    from mq_det_amd.modeling import pipeline
    g = torch.Generator().manual_seed(seed)
    C, nl = 256, len(sizes)
    items = []
    for l, (H, W) in enumerate(sizes):
        shapes = [(H, W)] + ([(H, W)] if l > 0 else []) + ([sizes[l + 1]] if l + 1 < nl else [])
        for k, (hs, ws) in enumerate(shapes):
            y = (torch.randn(B, hs * ws, C, generator=g) * (0.5 + 0.5 * k) + 0.2 * torch.randn(1, 1, C, generator=g)).to(dtype)
            if (hs, ws) == (H, W):
                w = torch.full((hs * ws,), 1.0 / (hs * ws), dtype=torch.float64)
            else:
                wy, wx = pipeline._upsample_pool_weights(hs, ws, H, W, torch.device("cpu"))
                w = (wy.double()[:, None] * wx.double()[None, :]).reshape(-1)
            items.append({"y": y.to(dev).contiguous(), "sums": _partials(y, w).to(dev), "n": hs * ws, "hs": hs, "ws": ws, "nbranches": len(shapes), "level": l,
                          "gamma": (1 + 0.2 * torch.randn(C, generator=g)).to(dtype).to(dev), "beta": (0.2 * torch.randn(C, generator=g)).to(dtype).to(dev)})
    r = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    return {"B": B, "sizes": sizes, "items": items, "dtype": dtype, "dev": dev,
            "attn_w": r(C, scale=1 / 16).to(dev), "attn_b": r(1, scale=0.5).to(dev),
            "w0": r(C // 4, C, scale=1 / 16).to(dtype).to(dev), "b0": r(C // 4, scale=0.3).to(dtype).to(dev),
            "w2": r(4 * C, C // 4, scale=1 / 4).to(dtype).to(dev), "b2": r(4 * C, scale=0.5).to(dtype).to(dev),
            "ln_w": (1 + 0.2 * r(C)).to(dtype).to(dev), "ln_b": (0.2 * r(C)).to(dtype).to(dev)}


def _levels(case, coefs, out):
    """the `levels` argument of ops.dyconv_epilogue_group / dyconv_fuse_act_group; out [B, N, C]: the levels are slices of it (batch stride N * C)"""
    lv, off = [], 0
    for l, (H, W) in enumerate(case["sizes"]):
        br = [(it["y"], cf, it["hs"], it["ws"]) for it, cf in zip(case["items"], coefs) if it["level"] == l]
        lv.append((br, H, W, out[:, off:off + H * W]))
        off += H * W
    return lv


def reference_relu_coef(case, coefs):
    """float64: the spatial mean of the UNROUNDED fused map built from the same y and coefficients, through the two FCs and the h_sigmoid
    normalisation of layers/dyrelu.py (lambda_a = 2, init_a = (1, 0), init_b = (0, 0)) -> [NL, B, 4, C]"""
    B, C = case["B"], 256
    out = []
    for l, (H, W) in enumerate(case["sizes"]):
        fused = torch.zeros(B, C, H, W, dtype=torch.float64)
        for it, cf in zip(case["items"], coefs):
            if it["level"] != l:
                continue
            y = it["y"].double().cpu().reshape(B, it["hs"], it["ws"], C).permute(0, 3, 1, 2)
            if (it["hs"], it["ws"]) != (H, W):
                y = F.interpolate(y, size=(H, W), mode="bilinear", align_corners=True)
            c64 = cf.double().cpu()
            fused += c64[:, :, 0, None, None] * y + c64[:, :, 1, None, None]
        m = fused.mean((2, 3))                                                                      # [B, C]
        h = torch.relu(m @ case["w0"].double().cpu().t() + case["b0"].double().cpu())
        z = h @ case["w2"].double().cpu().t() + case["b2"].double().cpu()                           # [B, 4C]
        hs = ((z + 3).clamp(0, 6) / 6).reshape(B, 4, C)
        out.append(torch.stack([(hs[:, 0] - 0.5) * 2 + 1, hs[:, 1] - 0.5, (hs[:, 2] - 0.5) * 2, hs[:, 3] - 0.5], 1))
    return torch.stack(out)


def run_case(B, sizes, dtype, dev, seed=0):
    """All four kernel checks on one pyramid; -> (e_old, e_new) of the DYReLU coefficients.  Raises AssertionError."""
    from mq_det_amd import ops
    case = make_case(B, sizes, dtype, dev, seed)
    items, nl, C = case["items"], len(sizes), 256
    N = sum(h * w for h, w in sizes)
    tag = f"B={B} {sizes} {dtype}"
    rw = (case["w0"], case["b0"], case["w2"], case["b2"])
    # 1. branch coefficients: bit-equal to mq_dyconv_coef_group
    coefs_old = ops.dyconv_coef_group(items, case["attn_w"], case["attn_b"], GROUPS, EPS_GN)
    coefs, rc_new = ops.dyconv_coef_relu_group(items, case["attn_w"], case["attn_b"], GROUPS, EPS_GN, *rw, nl)
    for k, (a, b) in enumerate(zip(coefs, coefs_old)):
        assert torch.equal(a, b), f"{tag}: coef of branch {k} differs from mq_dyconv_coef_group, max {float((a - b).abs().max()):.3e}"
    # today's path: fuse pass (pool partials) + DYReLU coefficients from them
    pre = torch.zeros(B, N, C, dtype=dtype, device=dev)
    rc_old = torch.empty(nl, B, 4, C, dtype=torch.float32, device=dev)
    ops.dyconv_epilogue_group(_levels(case, coefs_old, pre), *rw, rc_old)
    # 2. DYReLU coefficients against the float64 restatement
    ref = reference_relu_coef(case, coefs_old)
    e_old = float((rc_old.double().cpu() - ref).abs().max())
    e_new = float((rc_new.double().cpu() - ref).abs().max())
    print(f"dyrelu coefficients {tag}: e_old {e_old:.3e} e_new {e_new:.3e} (bound {max(1.5 * e_old, FLOOR):.3e})")
    assert e_new <= max(1.5 * e_old, FLOOR), f"{tag}: DYReLU coefficients e_new {e_new:.3e} > max(1.5 x e_old {e_old:.3e}, {FLOOR:.3e})"
    for name, rc in (("the pooled", rc_old), ("the analytic", rc_new)):
        # 3. mode LN == fuse, then DYReLU + LayerNorm (mq_dyrelu_ln_fwd), given the same relu_coef
        want = ops.dyrelu_layer_norm(pre, rc, sizes, case["ln_w"], case["ln_b"], EPS_LN)
        got = torch.full((B, N, C), float("nan"), dtype=dtype, device=dev)
        ops.dyconv_fuse_act_group(_levels(case, coefs, got), rc, case["ln_w"], case["ln_b"], EPS_LN)
        assert torch.equal(got, want), f"{tag}: mode LN with {name} coefficients differs, max {float((got.float() - want.float()).abs().max()):.3e}"
        # 4. mode ReLU == fuse, then mq_dyrelu_apply per level, on slices of one [B, N, 256] buffer
        want, off = pre.clone(), 0
        for l, (H, W) in enumerate(sizes):
            ops.dyrelu_apply_(want[:, off:off + H * W], rc[l])
            off += H * W
        got = torch.full((B, N, C), float("nan"), dtype=dtype, device=dev)
        ops.dyconv_fuse_act_group(_levels(case, coefs, got), rc)
        assert torch.equal(got, want), f"{tag}: mode ReLU with {name} coefficients differs, max {float((got.float() - want.float()).abs().max()):.3e}"
        # 5. mq_dyrelu_apply_group (all levels of the buffer in one launch) == mq_dyrelu_apply per level
        got = ops.dyrelu_apply_group_(pre.clone(), rc, sizes)
        assert torch.equal(got, want), f"{tag}: grouped DYReLU with {name} coefficients differs, max {float((got.float() - want.float()).abs().max()):.3e}"
    return e_old, e_new


def run_all(dev, dtypes=(torch.float16, torch.bfloat16)):
    out = []
    for dtype in dtypes:
        for i, (B, sizes) in enumerate(PYRAMIDS):
            out.append((str(dtype), B, sizes, *run_case(B, sizes, dtype, dev, seed=40 + i)))
    return out
