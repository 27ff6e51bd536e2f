"""TEST INFRASTRUCTURE ONLY.  The random-shape sweep of the kernels, split into DRAWING and RUNNING, so that the same draw runs through the
CPU emulation of the kernel sources (tests/test_simt_fuzz_cpu.py) and on the device (tests/test_gpu_fuzz.py), and a failing device draw
replays unchanged on the emulator (guard pages, gdb on a CPU build).

A FAMILY is one seeded stream of cases:

  FAMILIES[name].draws(rng, g, n, chip, **opt)  yields case dicts: the input tensors ON THE CPU, the parameters, "op" (which runner),
                                                "what" (label) and the tolerance(s).  Nothing in it touches a kernel.
  run(ops, case, put)                           calls the product on put(inputs), the tests/ops_emulation.py restatement on the CPU inputs
                                                and compares with `_close` / torch.equal.  `put` is the identity for the emulator and
                                                .to(device) for the GPU; outputs come back with .cpu().

A stream is made of ROUNDS: round r holds the base count of every operator of the family, in the order of the sweep's original test body
(n = 1: exactly the inputs that body drew).  More draws = more rounds, so draw k of a family is the same case whatever n is: the device's
draws (base count x 25) start with the emulator's, and `python tests/fuzz_cases.py <family> <k>` regenerates draw k from nothing else.

`chip` = {"cus": compute units, "f32": precise mode}: the Swin-MLP pass / tail draws place M around one and two full passes of THAT
machine (csrc/swin_mlp2.hip dispatch_swin_mlp2: workgroups per CU x tokens per workgroup); the emulator's "chip" has 4 CUs.

Operand modes (`cast_case`): "fp16" as drawn; "bf16" = every fp16 tensor rounded to bf16, tolerances x 8 (parity_checks.use_dtype);
"f32" = the precise mode (MQ_F32_OPERANDS=1): every fp16 tensor as a float, moved off the fp16 grid so that the low halves of the split
operands are not zero, tolerances min(stated, parity_checks.F32_TOL).  Tolerances named "ftol" belong to fp32 arithmetic on both sides
(scores, boxes, kernel-vs-kernel): they are the same in every mode.

Replay:  python tests/fuzz_cases.py <family> <draw> [--seed S] [--device cpu|cuda] [--dtype fp16|bf16|f32] [--env MQ_X=v ...] [--opt k=v ...]"""
import contextlib
import hashlib
import math
import os
import random
import struct
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

TOL = 2e-3
NMS_THRESH = 0.6
NMS_MARGIN = 1e-6            # a same-label pair of valid boxes whose float64 IoU is this close to the threshold: the case is not drawn
EMU_CHIP = {"cus": 4, "f32": False}


def _close(got, ref, what, tol=TOL):
    got, ref = got.float(), ref.float()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    scale = max(1.0, float(ref.abs().max()) if ref.numel() else 1.0)
    assert err == err and err <= tol * scale, f"{what}: max |err| {err:.3e} vs scale {scale:.3e} (tolerance {tol:.1e})"


def _edge(rng, tiles, hi):
    """a length at or next to a multiple of one of `tiles`, or anything in [1, hi]"""
    if rng.random() < 0.6:
        t = rng.choice(tiles)
        return max(1, min(hi, t * rng.randint(1, max(1, hi // t)) + rng.choice((-1, 0, 1))))
    return rng.randint(1, hi)


def swin_slot_tokens(C, chip):
    """tokens one full pass of mq_swin_mlp2_fwd's main kernel covers on `chip`: CUs x workgroups per CU x tokens per workgroup, the
    table of dispatch_swin_mlp2 (16-bit operands: 4 x 64 / 3 x 64 / 1 x 128; split-precise: 2 x 64 / 1 x 64 / 1 x 64)"""
    per_cu = {96: 2 * 64, 192: 64, 384: 64}[C] if chip.get("f32") else {96: 4 * 64, 192: 3 * 64, 384: 128}[C]
    return chip["cus"] * per_cu


SWIN_TAIL_ONLY_MAX_M = 30000       # flags & 4 sends every block through the 16-token tail kernel: check_swin_mlp caps those cases too


def nms_margin(boxes, labels, nvalid, thresh=NMS_THRESH):
    """smallest |IoU - thresh| over the same-label pairs of valid boxes, in float64 (the "+ 1" box convention of ml_nms)"""
    best = float("inf")
    for b in range(boxes.shape[0]):
        nv = int(nvalid[b])
        if nv < 2:
            continue
        bx, lab = boxes[b, :nv].double(), labels[b, :nv]
        area = (bx[:, 2] - bx[:, 0] + 1) * (bx[:, 3] - bx[:, 1] + 1)
        wh = (torch.min(bx[:, None, 2:], bx[None, :, 2:]) - torch.max(bx[:, None, :2], bx[None, :, :2]) + 1).clamp(min=0)
        inter = wh[..., 0] * wh[..., 1]
        d = (inter / (area[:, None] + area[None, :] - inter) - thresh).abs()
        d = d.masked_fill((lab[:, None] != lab[None, :]) | torch.eye(nv, dtype=torch.bool), float("inf"))
        best = min(best, float(d.min()))
    return best


# ------------------------------------------------------------------------------------------------------------------ drawing
def draws_attention(rng, g, n, chip):
    for _ in range(n):
        for _ in range(14):
            B, H, D = rng.randint(1, 3), rng.randint(1, 4), rng.choice((32, 64))
            Nq, Nk = _edge(rng, (16, 32, 128), 300), _edge(rng, (8, 16, 64, 256), 700)
            nsplit = rng.choice((1, 1, 2, 3, 5)) if Nk > 64 else 1
            clamp = rng.choice((0.0, 0.0, 50000.0))
            q = (torch.randn(B, Nq, H * D, generator=g) * rng.choice((1.0, 3.0))).half()
            k, v = torch.randn(B, Nk, H * D, generator=g).half(), torch.randn(B, Nk, H * D, generator=g).half()
            kb = kl = None
            if rng.random() < 0.6:                                       # padding-style mask: a tail of masked keys per batch item
                kb, kl = torch.zeros(B, Nk), torch.zeros(B, dtype=torch.int32)
                for b in range(B):
                    m = rng.randint(1, Nk)
                    kb[b, m:] = -1e30
                    kl[b] = m
                if rng.random() < 0.5 and Nk > 1:
                    kb[:, rng.randrange(1, Nk)] = -1e30                  # one more masked key, possibly inside the valid range (key 0 stays)
                    kl = None if rng.random() < 0.5 else kl              # (kv_len only promises that keys >= kv_len are masked by the bias)
                if kl is not None and rng.random() < 0.3:
                    kl = None
            yield dict(op="attention", q=q, k=k, v=v, H=H, D=D, kb=kb, kl=kl, clamp=clamp, nsplit=nsplit, tol=TOL,
                       what=f"attention: B={B} H={H} D={D} Nq={Nq} Nk={Nk} nsplit={nsplit} clamp={clamp} mask={kb is not None} kvlen={kl is not None}")


def draws_layernorm(rng, g, n, chip):
    for _ in range(n):
        for _ in range(16):
            C = 8 * rng.choice((1, 2, 12, 16, 17, 24, 32, 33, 48, 64, 65, 96, 128, 129, 192, 256, 257, 384))
            rows = _edge(rng, (4, 8, 16, 64), 300)
            x = torch.randn(rows, C, generator=g) * 2 + 0.3
            x = x if rng.random() < 0.5 else x.half()
            res = None
            if rng.random() < 0.6:
                res = torch.randn(rows, C, generator=g)
                res = res if rng.random() < 0.5 else res.half()
            w, b = (torch.randn(C, generator=g) * 0.1 + 1).half(), (torch.randn(C, generator=g) * 0.1).half()
            want_sum, want_y32 = rng.random() < 0.7, rng.random() < 0.5
            yield dict(op="layer_norm", x=x, res=res, w=w, b=b, want_sum=want_sum, want_y32=want_y32, clamp=0.0, tol=TOL,
                       what=f"layer_norm: rows={rows} C={C} x={x.dtype} res={None if res is None else res.dtype}")


def draws_vlfuse(rng, g, n, chip):
    it = 0
    for _ in range(n):
        for _ in range(6):
            B, Hh = rng.randint(1, 3), rng.choice((4, 8))
            N, T = _edge(rng, (16, 64, 128), 400), 8 * rng.randint(1, 32)
            kv = None if rng.random() < 0.4 else torch.tensor([rng.randint(1, T) for _ in range(B)], dtype=torch.int32)
            v_ln = torch.randn(B, N, 256, generator=g).half()
            kf = (torch.randn(B, Hh, T, 256, generator=g) / 8).half()
            vo = torch.randn(B, Hh, T, 256, generator=g).half()
            strided = bool(it % 2)                           # the pipeline's operands: views of ONE projection output (built by the runner)
            bias = torch.randn(B, Hh, T, generator=g)
            if kv is not None:
                for b in range(B):
                    bias[b, :, int(kv[b]):] = -1e30                      # the caller's bias masks the keys beyond kv_len
            if T > 2:
                bias[:, :, rng.randrange(T // 2)] = -1e30               # and one key inside the valid range
                bias[:, :, T // 2 if (kv is None or int(kv.min()) > T // 2) else 0] = 0.0
                if kv is not None:
                    for b in range(B):
                        if bool((bias[b, :, :int(kv[b])] < -1e29).all()):
                            bias[b, :, 0] = 0.0
            ob = torch.randn(256, generator=g).half()
            ns = rng.randint(1, 4)
            yield dict(op="vlfuse", v_ln=v_ln, kf=kf, vo=vo, strided=strided, bias=bias, ob=ob, kv=kv, ns=ns, tol=TOL,
                       what=f"vlfuse: B={B} heads={Hh} N={N} T={T} kv={None if kv is None else kv.tolist()} nsplit={ns} strided={strided}")
            it += 1


def draws_conv_dcn(rng, g, n, chip, full=True):
    """full False (MQ_OFFSET_CONV_VARIANT=2 in the emulator sweep): the offset conv only -- the stream then draws nothing for conv3x3 / DCNv2"""
    for _ in range(n):
        for _ in range(5):
            B, H, W = rng.randint(1, 2), _edge(rng, (8,), 27), _edge(rng, (16,), 37)
            C = rng.choice((64, 128, 256))
            x = torch.randn(B, H, W, C, generator=g).half()
            w27 = torch.zeros(32, 9 * C, dtype=torch.float16)
            w27[:27] = (torch.randn(27, 9 * C, generator=g) / 48).half()
            b27 = torch.randn(27, generator=g).half()
            case = dict(op="conv_dcn", x=x, w27=w27, b27=b27, dcn=False, tol=TOL, tol_conv=3e-3, tol_dcn=4e-3, what=f"offset conv / conv3x3 / dcnv2: {B}x{H}x{W}x{C}")
            if full and C == 256:
                stride = rng.choice((1, 2))
                w = (torch.randn(256, 9 * C, generator=g) / 48).half()
                bias = torch.randn(256, generator=g).half()
                Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
                om = torch.randn(B, 27, Ho, Wo, generator=g) * rng.choice((0.3, 2.0, 40.0))      # up to offsets far outside the image
                case.update(dcn=True, stride=stride, w=w, bias=bias, om=om.contiguous(), what=case["what"] + f" s{stride}")
            yield case


def _draw_align_scores(rng, g):
    B, HW, T = rng.randint(1, 3), _edge(rng, (4, 64), 200), rng.choice((16, 100, 255, 256))
    L, MT = _edge(rng, (64,), 90), rng.randint(1, 5)
    dot = (torch.randn(B, HW, T, generator=g) * 2)
    dot = dot if rng.random() < 0.5 else dot.half()
    tb, ctr = torch.randn(B, T, generator=g), torch.randn(B, HW, generator=g).half()
    tok = torch.full((L, MT), -1, dtype=torch.int32)
    for l in range(L):
        m = rng.randint(0, MT)
        tok[l, :m] = torch.tensor(rng.sample(range(T), m), dtype=torch.int32)
    return dict(op="align_scores", dot=dot, tb=tb, tok=tok, ctr=ctr, ftol=1e-5, what=f"align_scores: B={B} HW={HW} T={T} L={L} MT={MT}")


def _draw_nms(rng, g, stats):
    B, N = rng.randint(1, 3), _edge(rng, (64,), 900)
    xy = torch.rand(B, N, 2, generator=g) * 200
    boxes = torch.cat([xy, xy + 10 + torch.rand(B, N, 2, generator=g) * 60], -1).contiguous()
    labels = torch.randint(1, 4, (B, N), generator=g, dtype=torch.int32)
    nvalid = torch.tensor([rng.randint(0, N) for _ in range(B)], dtype=torch.int32)
    K = rng.randint(1, 200)
    stats["drawn"] = stats.get("drawn", 0) + 1
    if nms_margin(boxes, labels, nvalid) <= NMS_MARGIN:           # a pair ON the threshold: exact comparison undefined, not drawn
        stats["rejected"] = stats.get("rejected", 0) + 1
        return None
    return dict(op="ml_nms", boxes=boxes, labels=labels, nvalid=nvalid, K=K, what=f"ml_nms: B={B} N={N} nvalid={nvalid.tolist()} K={K}")


NMS_STATS = {}               # drawn / rejected counts of the last scoring_nms stream (the sweep asserts rejected <= 2 %)


def draws_scoring_nms(rng, g, n, chip):
    NMS_STATS.clear()
    for _ in range(n):
        for _ in range(8):
            yield _draw_align_scores(rng, g)
        for _ in range(4):
            case = _draw_nms(rng, g, NMS_STATS)
            if case is not None:
                yield case


def draws_sparse_window(rng, g, n, chip):
    for _ in range(n):
        for _ in range(5):
            B, T, V, S = rng.randint(1, 2), _edge(rng, (32,), 80), rng.randint(1, 60), rng.choice((1, 5, 8, 9, 16, 17, 25))
            q, kv = torch.randn(B, T, 512, generator=g).half(), torch.randn(B, V, 1024, generator=g).half()
            idx = torch.full((B, T, S), -1, dtype=torch.int32)
            for b in range(B):
                for t in range(T):
                    m = rng.choice((0, 0, S, rng.randint(0, S)))
                    m = min(m, V)
                    idx[b, t, :m] = torch.tensor(rng.sample(range(V), m), dtype=torch.int32)
            yield dict(op="gcp_sparse", q=q, kv=kv, idx=idx, tol=TOL, what=f"gcp_sparse: B={B} T={T} V={V} S={S}")
        for _ in range(4):
            ws, heads = rng.choice(((7, 3), (7, 6), (12, 3)))
            C = heads * 32
            B, H, W = rng.randint(1, 2), rng.randint(1, 2 * ws + 3), rng.randint(1, 2 * ws + 3)
            shift = rng.choice((0, ws // 2))
            qkv = torch.randn(B, H, W, 3 * C, generator=g).half()
            qb = torch.randn(3 * C, generator=g).half()
            rel = torch.randn(heads, ws * ws, ws * ws, generator=g)
            yield dict(op="window_attention", qkv=qkv, qb=qb, rel=rel, heads=heads, ws=ws, shift=shift, tol=3e-3,
                       what=f"window_attention: B={B} {H}x{W} ws={ws} heads={heads} shift={shift}")


def draws_round3_fused(rng, g, n, chip):
    """mq_window_attn_qkv_fwd (both widths: resident and streamed weights; images smaller than a window, several trips of the persistent
    workgroups, idle waves), mq_dyrelu_ln_fwd (1 .. 6 levels of ragged sizes) and mq_swin_mlp2_fwd across the pass / tail split."""
    for _ in range(n):
        for _ in range(6):
            heads = rng.choice((3, 6))
            C, ws = heads * 32, 7
            B, H, W = rng.randint(1, 3), rng.randint(1, 5 * ws + 3), rng.randint(1, 5 * ws + 3)
            shift = rng.choice((0, ws // 2))
            x = torch.randn(B, H, W, C, generator=g).half()
            w = (torch.randn(3 * C, C, generator=g) / math.sqrt(C)).half()
            bias = (torch.randn(3 * C, generator=g) * 0.2).half()
            rel = torch.randn(heads, ws * ws, ws * ws, generator=g) * 0.3
            yield dict(op="window_attention_qkv", x=x, w=w, bias=bias, rel=rel, heads=heads, ws=ws, shift=shift, tol=4e-3,
                       what=f"window_attention_qkv: B={B} {H}x{W} C={C} shift={shift}")
        for _ in range(6):
            nl = rng.randint(1, 6)
            sizes = [(rng.randint(1, 9), rng.randint(1, 11)) for _ in range(nl)]
            B, N = rng.randint(1, 3), sum(h * w_ for h, w_ in sizes)
            big = torch.randn(B, N + 5, 256, generator=g).half() * 2          # rows of a larger buffer: batch stride != N * C
            coef = torch.randn(nl, B, 4, 256, generator=g)
            gam, bet = (torch.randn(256, generator=g) * 0.1 + 1).half(), (torch.randn(256, generator=g) * 0.1).half()
            yield dict(op="dyrelu_layer_norm", big=big, coef=coef, sizes=sizes, gam=gam, bet=bet, tol=4e-3, what=f"dyrelu_layer_norm: B={B} sizes={sizes}")
        for _ in range(4):
            C = rng.choice((96, 192, 384))
            # lengths around one and two full passes of the chip (the emulator's has 4 CUs: 16 / 12 / 4 workgroup slots of 64 / 64 / 128 tokens)
            slot = swin_slot_tokens(C, chip)
            M = max(1, slot * rng.choice((1, 1, 2)) + rng.choice((-17, -1, 0, 1, 15, 16, 33, 70)))
            x = torch.randn(M, C, generator=g)
            delta = (torch.randn(M, C, generator=g) * 0.5).half() if rng.random() < 0.7 else None
            lg_, lb_ = (torch.randn(C, generator=g) * 0.1 + 1).half(), (torch.randn(C, generator=g) * 0.1).half()
            w1, b1 = (torch.randn(4 * C, C, generator=g) / math.sqrt(C)).half(), (torch.randn(4 * C, generator=g) * 0.1).half()
            w2, b2 = (torch.randn(C, 4 * C, generator=g) / math.sqrt(4 * C)).half(), (torch.randn(C, generator=g) * 0.1).half()
            nln = (lg_, lb_, 1e-5) if rng.random() < 0.7 else None
            flags = rng.choice((0, 2, 1, 4))
            if flags & 4 and M > SWIN_TAIL_ONLY_MAX_M:                   # (never on the emulator's chip)
                M = SWIN_TAIL_ONLY_MAX_M
                x, delta = x[:M].contiguous(), None if delta is None else delta[:M].contiguous()
            yield dict(op="swin_mlp2", x=x, delta=delta, lg=lg_, lb=lb_, w1=w1, b1=b1, w2=w2, b2=b2, nln=nln, flags=flags, tol=3e-3, tol_next=3e-3,
                       what=f"swin_mlp2 (pass / tail split): C={C} M={M} flags={flags} delta={delta is not None} next={nln is not None}")


def draws_round4(rng, g, n, chip):
    """mq_attn_text_fwd (caption lengths around every 16-key block and the 160-key variant switch, per-item kv_len, max_kv above / at / absent,
    clamp, D = 32 / 64), mq_patch_embed_fwd (both pixel layouts, widths around multiples of 16 patches, C = 96 / 192), and the
    post-processing kernels (mq_post_select_fwd over one / several slices with scores quantised so that ties straddle every cut,
    mq_post_sort_fwd, mq_post_finalize_fwd)."""
    for _ in range(n):
        for _ in range(8):
            B, H, D = rng.randint(1, 3), rng.randint(1, 4), rng.choice((32, 64))
            T = rng.choice((256, 256, 8 * rng.randint(1, 32)))
            kv = max(1, min(T, _edge(rng, (16, 32, 160), T)))
            clamp = rng.choice((0.0, 0.0, 50000.0, 2.5))
            qkv = (torch.randn(B, T, 3 * H * D, generator=g) * rng.choice((1.0, 4.0))).half()
            kl = torch.tensor([max(1, kv - rng.randint(0, 20) * (b > 0)) for b in range(B)], dtype=torch.int32)
            kb = torch.zeros(B, T)
            for b in range(B):
                kb[b, int(kl[b]):] = -1e30
            mk = rng.choice((0, kv, min(T, kv + rng.randint(0, 40))))
            use_kl = rng.random() < 0.8
            yield dict(op="attention_text", qkv=qkv, H=H, kb=kb, kl=kl, use_kl=use_kl, mk=mk, clamp=clamp, tol=TOL,
                       what=f"attention_text: B={B} H={H} D={D} T={T} kv={kv} max_kv={mk} clamp={clamp} kv_len={use_kl}")
        for _ in range(6):
            C = rng.choice((96, 192))
            B, Hi, Wi = rng.randint(1, 2), 4 * rng.randint(1, 9), 4 * _edge(rng, (16,), 70)
            img = torch.randn(B, 3, Hi, Wi, generator=g).half()
            w = (torch.randn(C, 3, 4, 4, generator=g) * 0.2).half()
            prm = [torch.randn(C, generator=g) * s_ + o_ for s_, o_ in ((0.1, 0), (0.2, 1), (0.1, 0), (0.2, 1), (0.1, 0))]
            nchw = rng.random() < 0.5
            yield dict(op="patch_embed", img=img, w=w, prm=prm, nchw=nchw, tol=2e-3, what=f"patch_embed: B={B} {Hi}x{Wi} C={C} {'fp32 NCHW' if nchw else 'NHWC'}")
        for it in range(5):
            B, L, nl = rng.randint(1, 2), rng.randint(1, 12), rng.randint(1, 4)
            shapes = [(rng.randint(1, 40), rng.randint(1, 90)) for _ in range(nl)]
            if it % 2 == 0:
                shapes[0] = (rng.randint(60, 75), rng.randint(60, 75))           # > 32768 scores with L >= 8: several slices
                L = max(L, 8)
            topn = rng.choice((1, 17, 300, 1000, 1500))
            quant = rng.choice((None, 3, 40))
            dens = rng.choice((0.0, 0.02, 0.5, 1.0))
            ranked, reg, anchors, ks = [], [], [], []
            for (h, w_) in shapes:
                hw = h * w_
                v = torch.rand(B, hw, L, generator=g)
                if quant:
                    v = (torch.floor(v * quant) + 1) / (quant + 1)
                ranked.append(torch.where(torch.rand(B, hw, L, generator=g) < dens, v, torch.full_like(v, -1.0)).contiguous())
                reg.append((torch.randn(B, hw, 4, generator=g) * 2).contiguous())
                xy = torch.rand(hw, 2, generator=g) * 300
                anchors.append(torch.cat([xy, xy + 8 + torch.rand(hw, 2, generator=g) * 64], 1).contiguous())
                ks.append(min(topn, hw * L))
            lab = torch.randperm(L, generator=g).to(torch.int32) + 1
            wh = torch.tensor([[333.0, 250.0]] * B)
            tot = sum(ks)
            K = rng.randint(1, tot)
            K2 = min(tot, K + rng.choice((0, 1, 16)))
            keep = (torch.rand(B, tot, generator=g) < rng.choice((0.1, 0.7, 1.0))).to(torch.uint8)
            yield dict(op="post", ranked=ranked, reg=reg, anchors=anchors, ks=ks, lab=lab, wh=wh, shapes=shapes, B=B, L=L, K=K, K2=K2, keep=keep,
                       what=f"post: B={B} shapes={shapes} L={L} k={ks} quant={quant} dens={dens} K={K} K2={K2}")


def draws_grouped_dyconv(rng, g, n, chip):
    """mq_conv3x3_nchw32_group_fwd and mq_dyconv_epilogue_group on random pyramids (1 .. 6 levels, level sizes around the 8 x 16 tile and
    the 128-position block edges, levels as slices of one token buffer, B = 1 .. 3)."""
    for _ in range(n):
        for _ in range(3):
            B, nl = rng.randint(1, 3), rng.randint(1, 6)
            sizes = [(_edge(rng, (8, 16), 24), _edge(rng, (16, 32), 40)) for _ in range(nl)]
            tok = torch.randn(B, sum(h * w_ for h, w_ in sizes) + 3, 256, generator=g).half()
            w = (torch.randn(27, 256, 3, 3, generator=g) / 48).half()
            bias = torch.randn(27, generator=g).half()
            yield dict(op="conv_group", tok=tok, w=w, bias=bias, sizes=sizes, ftol_level=2e-6, ftol=1e-5, what=f"offset conv group: B={B} sizes={sizes}")
        for _ in range(3):
            B, nl = rng.randint(1, 3), rng.randint(1, 5)
            sizes = [(rng.randint(1, 14), _edge(rng, (16,), 20)) for _ in range(nl)]
            w0, b0 = (torch.randn(64, 256, generator=g) / 16).half(), (torch.randn(64, generator=g) * 0.1).half()
            w2, b2 = (torch.randn(1024, 64, generator=g) / 8).half(), (torch.randn(1024, generator=g) * 0.1).half()
            levels = []
            for (h, w_) in sizes:
                branches = []
                for _ in range(rng.randint(0, 3) if rng.random() < 0.7 else 0):
                    branches.append(((torch.randn(B, h * w_, 256, generator=g)).half(), torch.randn(B, 256, 2, generator=g) * 0.5, h, w_))
                if not branches or (len(branches) < 3 and rng.random() < 0.6):
                    hs, ws = max(1, (h + 1) // 2), max(1, (w_ + 1) // 2)
                    if (hs, ws) == (h, w_) or len(branches) == 0 and rng.random() < 0.3:
                        branches.append((torch.randn(B, h * w_, 256, generator=g).half(), torch.randn(B, 256, 2, generator=g) * 0.5, h, w_))
                    else:
                        branches.insert(rng.randint(0, len(branches)), (torch.randn(B, hs * ws, 256, generator=g).half(), torch.randn(B, 256, 2, generator=g) * 0.5, hs, ws))
                levels.append([list(br) for br in branches])
            yield dict(op="epilogue_group", B=B, sizes=sizes, w0=w0, b0=b0, w2=w2, b2=b2, levels=levels,
                       what=f"epilogue group: B={B} sizes={sizes} branches={[len(l_) for l_ in levels]}")


def draws_swin_roi_msda(rng, g, n, chip):
    for _ in range(n):
        for _ in range(4):
            C, M = rng.choice((96, 192, 384)), _edge(rng, (16, 32, 64, 128), 400)
            x = torch.randn(M, C, generator=g) * 1.5
            delta = (torch.randn(M, C, generator=g) * 0.5).half() if rng.random() < 0.7 else None
            lg, lb = (torch.randn(C, generator=g) * 0.1 + 1).half(), (torch.randn(C, generator=g) * 0.1).half()
            w1, b1 = (torch.randn(4 * C, C, generator=g) / math.sqrt(C)).half(), (torch.randn(4 * C, generator=g) * 0.1).half()
            w2, b2 = (torch.randn(C, 4 * C, generator=g) / math.sqrt(4 * C)).half(), (torch.randn(C, generator=g) * 0.1).half()
            nxt = ((torch.randn(C, generator=g) * 0.1 + 1).half(), (torch.randn(C, generator=g) * 0.1).half(), 1e-5) if rng.random() < 0.6 else None
            flags = rng.choice((0, 1, 2, 4))
            yield dict(op="swin_mlp2", x=x, delta=delta, lg=lg, lb=lb, w1=w1, b1=b1, w2=w2, b2=b2, nln=nxt, flags=flags, tol=1e-3, tol_next=2e-3,
                       what=f"swin_mlp2: C={C} M={M} flags={flags} delta={delta is not None} next={nxt is not None}")
        for _ in range(4):
            N, C, H, W = rng.randint(1, 2), rng.choice((8, 64, 256)), rng.randint(1, 30), rng.randint(1, 40)
            feat = torch.randn(N, C, H, W, generator=g)
            R = rng.randint(1, 9)
            x1, y1 = torch.rand(R, generator=g) * W * 16 - 24, torch.rand(R, generator=g) * H * 16 - 24     # partly outside the image
            rois = torch.stack([torch.randint(0, N, (R,), generator=g).float(), x1, y1, x1 + torch.rand(R, generator=g) * 200,
                                y1 + torch.rand(R, generator=g) * 200], 1)
            srs = [rng.choice((0, 2)) for _ in range(2)]
            yield dict(op="roi_align", feat=feat, rois=rois, srs=srs, ftol=1e-4, what=f"roi_align: {N}x{C}x{H}x{W} R={R} sr={srs}")
        for _ in range(3):
            B, M, D = rng.randint(1, 2), 8, 32
            shapes = [(rng.randint(2, 14), rng.randint(2, 18)) for _ in range(4)]
            S, Q = sum(h * w for h, w in shapes), _edge(rng, (4, 64), 150)
            value = torch.randn(B, S, M * D, generator=g).half()
            qp = torch.cat([torch.randn(B, Q, M * 16 * 2, generator=g) * 3.0, torch.randn(B, Q, M * 16, generator=g)], -1).half()
            nd = rng.choice((2, 4))
            ref_pts = torch.rand(B, Q, 4, nd, generator=g) * 1.2 - 0.1                                   # some reference points outside [0, 1]
            if nd == 4:
                ref_pts[..., 2:] = ref_pts[..., 2:].abs() * 0.3 + 0.02
            vhw = None
            if rng.random() < 0.5:
                vhw = torch.tensor([[[rng.randint(1, h), rng.randint(1, w)] for (h, w) in shapes] for _ in range(B)], dtype=torch.int32)
            yield dict(op="msda_q", value=value, shapes=shapes, qp=qp, ref_pts=ref_pts, M=M, vhw=vhw, tol=TOL,
                       what=f"ms_deform_attn_q: B={B} shapes={shapes} Q={Q} ref_dim={nd} valid_hw={vhw is not None}")


def draws_bf16_twins(rng, g, n, chip):
    """the *_bf16 entry points on draws of their own (tolerance x 8): attention once per MQ_ATTN_RESIDENT setting, LayerNorm once per MQ_LN_VARIANT"""
    bf = torch.bfloat16
    for _ in range(n):
        for res_attn in (0, 1):
            for _ in range(5):
                B, H, D = rng.randint(1, 2), rng.randint(1, 3), rng.choice((32, 64))
                Nq, Nk = _edge(rng, (16, 32, 128), 200), _edge(rng, (8, 16, 64, 256), 500)
                q, k, v = (torch.randn(B, m, H * D, generator=g).to(bf) for m in (Nq, Nk, Nk))
                yield dict(op="attention", q=q, k=k, v=v, H=H, D=D, kb=None, kl=None, clamp=0.0, nsplit=1, tol=8 * TOL, sel={"ATTN_RESIDENT": res_attn},
                           what=f"attention bf16 (resident={res_attn}): B={B} H={H} D={D} Nq={Nq} Nk={Nk}")
        for variant in (1, 2):
            for _ in range(5):
                C, rows = 8 * rng.choice((12, 24, 32, 48, 96, 192)), _edge(rng, (4, 16), 200)
                x, res = torch.randn(rows, C, generator=g) * 2, torch.randn(rows, C, generator=g).to(bf)
                w, b = (torch.randn(C, generator=g) * 0.1 + 1).to(bf), (torch.randn(C, generator=g) * 0.1).to(bf)
                yield dict(op="layer_norm", x=x, res=res, w=w, b=b, want_sum=True, want_y32=True, clamp=0.0, tol=8 * TOL, sel={"LN_VARIANT": variant},
                           what=f"layer_norm bf16 [v{variant}]: rows={rows} C={C}")


# ---- families the emulator sweep did not have (base counts sized for the emulator; tolerances: the rows of tests/parity_checks.py)
def draws_clamped(rng, g, n, chip):
    """layer_norm(..., clamp > 0) (mq_layernorm_clamp_fwd) and clamp_gelu_clamp on values that DO reach the clamp (|x| up to ~ 4 clamp);
    tolerance: check_bert_clamp_fused (TOL)"""
    for _ in range(n):
        for _ in range(6):
            C = 8 * rng.choice((1, 12, 17, 32, 96, 129, 384))
            rows = _edge(rng, (4, 8, 16, 64), 200)
            clamp = rng.choice((0.5, 2.0, 50000.0))
            amp = clamp * rng.choice((0.5, 1.5, 4.0)) if clamp < 100 else 20000.0
            x = torch.randn(rows, C, generator=g) * amp
            x = x if rng.random() < 0.5 else x.half()
            res = None
            if rng.random() < 0.6:
                res = torch.randn(rows, C, generator=g) * min(amp, 4.0)
                res = res if rng.random() < 0.5 else res.half()
            w = (torch.randn(C, generator=g) * (clamp if clamp < 100 else 1.0) + 1).half()       # |gamma| large enough for y to reach the clamp
            b = (torch.randn(C, generator=g) * 0.1).half()
            want_sum, want_y32 = rng.random() < 0.7, rng.random() < 0.5
            yield dict(op="layer_norm", x=x, res=res, w=w, b=b, want_sum=want_sum, want_y32=want_y32, clamp=clamp, tol=TOL,
                       what=f"layer_norm clamp={clamp}: rows={rows} C={C} amp={amp} x={x.dtype} res={None if res is None else res.dtype}")
        for _ in range(6):
            numel = 8 * _edge(rng, (8, 32, 128), 4000)
            clamp = rng.choice((0.5, 3.0, 50000.0))
            x = (torch.randn(numel, generator=g) * (clamp * 2 if clamp < 100 else 30000.0)).half()
            yield dict(op="clamp_gelu_clamp", x=x, clamp=clamp, tol=TOL, what=f"clamp_gelu_clamp: n={numel} clamp={clamp}")


def draws_patch_merge(rng, g, n, chip):
    """mq_patch_merge_ln_fwd: odd H / W (the zero-padded row / column), C = 96 .. 768, fp32 and 16-bit input; tolerance: the 1e-3 of
    test_gpu_parity._body_patch_merge_ln_kernel against the torch statement"""
    for _ in range(n):
        for _ in range(6):
            C = rng.choice((96, 192, 384, 768))
            B, H, W = rng.randint(1, 3), rng.randint(1, 13), _edge(rng, (2, 8), 21)
            x = torch.randn(B, H, W, C, generator=g) * 2 + 0.3
            x = x if rng.random() < 0.5 else x.half()
            w, b = (torch.randn(4 * C, generator=g) * 0.1 + 1).half(), (torch.randn(4 * C, generator=g) * 0.1).half()
            yield dict(op="patch_merge_ln", x=x, w=w, b=b, tol=1e-3, what=f"patch_merge_ln: B={B} {H}x{W} C={C} x={x.dtype}")


def draws_pyramid_elementwise(rng, g, n, chip):
    """pool2x2_tokens (1 .. 5 levels, odd sizes: bit for bit the torch statement), add_upsample_nearest_ (H, W in {2 Hc, 2 Hc - 1}),
    dyrelu_apply_ (one rounding of the fp32 result: TOL) and box_decode (fp32: 1e-6 boxes / 2e-7 scores as the post family, labels exact)"""
    for _ in range(n):
        for _ in range(4):
            B, nl = rng.randint(1, 3), rng.randint(1, 5)
            sizes = [(rng.randint(2, 23), rng.randint(2, 35)) for _ in range(nl)]
            feats = [torch.randn(B, h, w, 256, generator=g).half() for h, w in sizes]
            yield dict(op="pool2x2_tokens", feats=feats, what=f"pool2x2_tokens: B={B} sizes={sizes}")
        for _ in range(4):
            B, C = rng.randint(1, 3), rng.choice((64, 256))
            Hc, Wc = rng.randint(1, 14), _edge(rng, (8,), 20)
            H, W = 2 * Hc - rng.randint(0, 1), 2 * Wc - rng.randint(0, 1)
            dst, src = torch.randn(B, H, W, C, generator=g).half(), torch.randn(B, Hc, Wc, C, generator=g).half()
            yield dict(op="add_upsample", dst=dst, src=src, tol=TOL, what=f"add_upsample_nearest_: B={B} {H}x{W} <- {Hc}x{Wc} C={C}")
        for _ in range(4):
            B, N = rng.randint(1, 3), _edge(rng, (4, 64), 300)
            x = (torch.randn(B, N, 256, generator=g) * 2).half()
            coef = torch.randn(B, 4, 256, generator=g)
            yield dict(op="dyrelu_apply", x=x, coef=coef, tol=TOL, what=f"dyrelu_apply_: B={B} N={N}")
        for _ in range(4):
            B, L, HW = rng.randint(1, 3), rng.randint(1, 12), _edge(rng, (64,), 400)
            K, off = rng.randint(1, min(300, HW * L)), rng.randint(0, 40)
            val = torch.rand(B, K, generator=g)
            val = torch.where(torch.rand(B, K, generator=g) < 0.2, torch.full_like(val, -1.0), val)          # empty candidate slots
            flat = torch.randint(0, HW * L, (B, K), generator=g)
            reg = (torch.randn(B, HW, 4, generator=g) * rng.choice((0.5, 2.0, 12.0))).contiguous()          # up to the exp clamp of the decoder
            xy = torch.rand(HW, 2, generator=g) * 300
            anchors = torch.cat([xy, xy + 8 + torch.rand(HW, 2, generator=g) * 64], 1).contiguous()
            reg = reg if rng.random() < 0.5 else reg.half()
            lab = torch.randperm(L, generator=g).to(torch.int32) + 1
            wh = torch.tensor([[333.0, 250.0]] * B)
            yield dict(op="box_decode", val=val, flat=flat, reg=reg, anchors=anchors, lab=lab, wh=wh, HW=HW, L=L, off=off, tot=off + K + rng.randint(0, 9),
                       ftol=1e-6, ftol_score=2e-7, what=f"box_decode: B={B} HW={HW} L={L} K={K} off={off}")


def draws_vlfuse_masked(rng, g, n, chip):
    """mq_vlfuse_t2i_fwd with an image key mask (MQ-GroundingDINO: padded image tokens; a padding tail per image and single masked tokens inside),
    4 and 8 heads, key splits with splits that are masked out entirely; tolerance: TOL (gdino_checks.check_vlfuse_heads_mask)"""
    for _ in range(n):
        for _ in range(4):
            B, Hh = rng.randint(1, 3), rng.choice((4, 8))
            N, T = _edge(rng, (16, 64, 128), 400), 8 * rng.randint(1, 32)
            kv = None if rng.random() < 0.4 else torch.tensor([rng.randint(1, T) for _ in range(B)], dtype=torch.int32)
            v_ln = torch.randn(B, N, 256, generator=g).half()
            kf = (torch.randn(B, Hh, T, 256, generator=g) / 8).half()
            mask = torch.zeros(B, N, dtype=torch.bool)
            for b in range(B):
                mask[b, rng.randint(1, N):] = True                     # padding tail (token 0 stays live)
                if N > 2 and rng.random() < 0.5:
                    mask[b, rng.randrange(1, N)] = True
            ns = rng.randint(1, 4)
            yield dict(op="vlfuse", parts=("t2i",), v_ln=v_ln, kf=kf, vo=None, strided=False, bias=None, ob=None, kv=kv, ns=ns, mask=mask, tol=TOL,
                       what=f"vlfuse_t2i key_mask: B={B} heads={Hh} N={N} T={T} kv={None if kv is None else kv.tolist()} nsplit={ns} live={[int((~m).sum()) for m in mask]}")


# ---- the fused text / head kernels and the DCNv2 statistics / grouped launch (tolerances: the rows of tests/parity_checks.py named in each docstring)
BERT_C, BERT_HEADS = 768, 12         # BERT-base and the tiny spec alike (oracle/spec.py: bert_hidden / bert_heads): the one width mq_bert_attn_qkv_fwd takes


def draws_bert_qkv(rng, g, n, chip):
    """mq_bert_attn_qkv_fwd: T around every 16-key block and the 160-token variant switch, kv_len per item, clamp (with logits AT the clamp),
    hidden states as a view with padded row stride, weights packed by the caller or by the wrapper.  Draws that bert_attention_qkv_fits refuses
    (precise mode: T > 160) are left out by `served`.  Tolerance: check_bert_attn_qkv (TOL)."""
    C = BERT_C
    for _ in range(n):
        for _ in range(3):
            B, T = rng.randint(1, 2), _edge(rng, (16, 160), 256)
            kv = max(1, min(T, _edge(rng, (16,), T)))
            clamp, amp = rng.choice(((0.0, 1.0), (50000.0, 1.0), (3.0, 8.0)))
            xs = torch.randn(B, T, C + 8, generator=g).half()
            w = torch.randn(3 * C, C, generator=g) / math.sqrt(C)
            w[:2 * C] *= amp                                               # q and k only: logits that reach the clamp, values of unit size
            w, bq = w.half(), (torch.randn(3 * C, generator=g) * 0.1).half()
            kl = torch.tensor([max(1, kv - rng.randint(0, 20) * (b > 0)) for b in range(B)], dtype=torch.int32)
            kb = torch.zeros(B, T)
            for b in range(B):
                kb[b, int(kl[b]):] = -1e30
            use_kl, packed = rng.random() < 0.7, rng.random() < 0.5
            yield dict(op="bert_qkv", xs=xs, w=w, bq=bq, kb=kb, kl=kl, use_kl=use_kl, packed=packed, clamp=clamp, tol=TOL,
                       what=f"bert_attention_qkv: B={B} T={T} kv={kl.tolist()} clamp={clamp} amp={amp} kv_len={use_kl} packed={packed}")


def draws_gcp_fused(rng, g, n, chip):
    """mq_gcp_attn_fwd (T, V, S as the sparse-attention draws; rows without a live index: x_out == x bit for bit; want_gate; with / without the
    trailing LayerNorm; every rows_per_block; packed weights) and mq_gcp_gate_residual_fwd (fp32 and 16-bit stream).  S = 9 is there for the
    predicate: draws gcp_attention_fits refuses are left out by `served`.  Tolerances: check_gcp_attn_fused (2e-3 stream / LN_f, 4e-3 gate);
    the gate kernel is one rounding of an fp32 result (TOL)."""
    for _ in range(n):
        for _ in range(2):
            B, T, V, S = rng.randint(1, 2), _edge(rng, (16, 32), 80), rng.randint(1, 60), rng.choice((1, 3, 5, 8, 8, 9))
            x = torch.randn(B, T, 768, generator=g) * 1.5
            kv = torch.randn(B, V, 1024, generator=g).half()
            idx = torch.full((B, T, S), -1, dtype=torch.int32)
            for b in range(B):
                for t in range(T):
                    m = min(rng.choice((0, 0, S, rng.randint(0, S))), V)
                    idx[b, t, :m] = torch.tensor(rng.sample(range(V), m), dtype=torch.int32)
            wq = (torch.randn(512, 768, generator=g) / 768 ** 0.5).half()
            wout = (torch.randn(768, 512, generator=g) / 512 ** 0.5).half()
            wg1 = (torch.randn(384, 768, generator=g) / 768 ** 0.5).half()
            w2 = (torch.randn(384, generator=g) * 0.1).half()
            lns = [[(torch.rand(768, generator=g) + 0.5).half(), (torch.randn(768, generator=g) * 0.1).half()] for _ in range(3)]
            lnf, want_gate, rb, packed = rng.random() < 0.6, rng.random() < 0.6, rng.choice((0, 16, 32)), rng.random() < 0.5
            yield dict(op="gcp_attention", x=x, kv=kv, idx=idx, wq=wq, wout=wout, wg1=wg1, w2=w2, lns=lns, lnf=lnf, want_gate=want_gate, rb=rb, packed=packed,
                       tol=2e-3, tol_gate=4e-3, what=f"gcp_attention: B={B} T={T} V={V} S={S} ln_f={lnf} gate={want_gate} rows/block={rb} packed={packed}")
        for _ in range(2):
            M = _edge(rng, (4, 16, 64), 200)
            sup, h = torch.randn(M, 768, generator=g).half(), torch.randn(M, 384, generator=g).half()
            w2 = (torch.randn(384, generator=g) * 0.1).half()
            x = torch.randn(M, 768, generator=g) * 1.5
            x32, want_gate = rng.random() < 0.5, rng.random() < 0.5
            yield dict(op="gcp_gate_residual", sup=sup, h=h, w2=w2, x=x if x32 else x.half(), want_gate=want_gate, tol=TOL, ftol=1e-5,
                       what=f"gcp_gate_residual: M={M} stream={'fp32' if x32 else '16-bit'} gate={want_gate}")


def draws_align_fused(rng, g, n, chip):
    """mq_align_fused_fwd: 1 .. 5 ragged levels (tiles that straddle levels, last tiles of a few rows), T in 16 / 100 / 255 / 256, kv_max absent /
    at / above the live tokens, one caption per batch or per item, agg 0 / 1 / 2.  Scores within the row's tolerance of the threshold may fall
    either way (the `far` masking of the align_scores family, at this row's 1e-3).  Draws align_fused_fits refuses (precise mode: more than
    144 live tokens) are left out by `served`.  Tolerances: check_align_fused (1e-3 logits / centerness / class / ranked, 2e-3 box deltas)."""
    for _ in range(n):
        for _ in range(4):
            B, nl, T = rng.randint(1, 3), rng.randint(1, 5), rng.choice((16, 100, 255, 256))
            sizes = [(rng.randint(1, 9), _edge(rng, (4, 16), 13)) for _ in range(nl)]
            N = sum(h * w_ for h, w_ in sizes)
            nv = rng.randint(1, T)
            kv_max = rng.choice((0, nv, min(T, nv + rng.randint(1, 40))))
            L, MT, agg, per_item = rng.randint(1, 40), rng.randint(1, 5), rng.choice((0, 1, 2)), rng.random() < 0.4
            tok = (torch.randn(B, N, 256, generator=g) * 0.7).half()
            tk = (torch.randn(B, T, 256, generator=g) * 0.12).half()
            tbias = torch.randn(B, T, generator=g) * 0.5 - 1.0
            wbc = torch.zeros(16, 256)
            wbc[:5] = torch.randn(5, 256, generator=g) * 0.05
            bbc = torch.cat([torch.randn(5, generator=g) * 0.1, torch.zeros(3)])
            scales = torch.rand(nl, generator=g) + 0.5
            tokidx = torch.full((B, L, MT) if per_item else (L, MT), -1, dtype=torch.int32)
            for row in tokidx.view(-1, MT):
                m = min(rng.randint(0, MT), nv)
                row[:m] = torch.tensor(rng.sample(range(nv), m), dtype=torch.int32)
            yield dict(op="align_fused", tok=tok, tk=tk, tbias=tbias, wbc=wbc.half(), bbc=bbc, scales=scales, tokidx=tokidx, sizes=sizes, agg=agg, kv_max=kv_max,
                       nv=nv, tol=1e-3, tol_reg=2e-3,
                       what=f"align_fused: B={B} sizes={sizes} T={T} live={nv} kv_max={kv_max} L={L} MT={MT} agg={agg} per_item={per_item}")


def _draw_dcn_branch(rng, g, B):
    H, W, stride = _edge(rng, (8,), 12), _edge(rng, (16,), 18), rng.choice((1, 2))
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = torch.randn(B, H, W, 256, generator=g).half()
    w, bias = (torch.randn(256, 9 * 256, generator=g) / 48).half(), torch.randn(256, generator=g).half()
    om = (torch.randn(B, 27, Ho, Wo, generator=g) * rng.choice((0.3, 2.0, 40.0))).contiguous()
    wy, wx = (torch.rand(Ho, generator=g), torch.rand(Wo, generator=g)) if rng.random() < 0.6 else (None, None)
    return dict(x=x, om=om, w=w, bias=bias, stride=stride, wy=wy, wx=wx), f"{H}x{W}s{stride}{'w' if wy is not None else ''}"


def draws_dcn_stats_group(rng, g, n, chip):
    """mq_dcnv2_fwd with want_stats (the GroupNorm / scale-attention sums of its epilogue against the same sums over the kernel's OWN output, as
    check_dcn does: 1e-4; the output against the restatement: 4e-3) and mq_dcnv2_group_fwd with 1 .. 4 branches of mixed stride and size
    (bit for bit the single launch, output and sums -- check_dcn's tol 0 rows)."""
    for _ in range(n):
        for _ in range(2):
            B = rng.randint(1, 2)
            br, tag = _draw_dcn_branch(rng, g, B)
            yield dict(op="dcn_stats", br=br, tol_dcn=4e-3, tol_stats=1e-4, what=f"dcnv2 want_stats: B={B} {tag}")
        for _ in range(2):
            B, nb = rng.randint(1, 2), rng.randint(1, 4)
            brs = [_draw_dcn_branch(rng, g, B) for _ in range(nb)]
            yield dict(op="dcn_group", brs=[b_ for b_, _ in brs], tol_dcn=4e-3, what=f"dcnv2_group: B={B} branches={[t for _, t in brs]}")


# ------------------------------------------------------------------------------------------------------------------ running
@contextlib.contextmanager
def _selected(ops, sel):
    """the live kernel selection with `sel` on top, for one call (what monkeypatch.setenv + ops.configure() did in the original sweep)"""
    saved = {k: ops.KERNELS[k] for k in (sel or {})}
    ops.KERNELS.update(sel or {})
    try:
        yield
    finally:
        ops.KERNELS.update(saved)


def _tup(x):
    return x if isinstance(x, tuple) else (x,)


def _run_attention(ops, emu, c, put):
    q, k, v, H, D = c["q"], c["k"], c["v"], c["H"], c["D"]
    B, Nq, Nk = q.shape[0], q.shape[1], k.shape[1]
    vt = F.pad(v, (0, 0, 0, (-Nk) % 8)).transpose(1, 2).contiguous()
    ref = emu.attention4(q.view(B, Nq, H, D), k.view(B, Nk, H, D), vt.view(B, H, D, -1), c["kb"], None, c["clamp"], nk=Nk)
    with _selected(ops, c.get("sel")):
        got = ops.attention(put(q), put(k), put(vt), H, D, key_bias=put(c["kb"]), clamp=c["clamp"], nsplit=c["nsplit"], nk=Nk, kv_len=put(c["kl"])).cpu()
    assert got.dtype == q.dtype
    _close(got, ref, c["what"], c["tol"])


def _run_layer_norm(ops, emu, c, put):
    kw = dict(residual=c["res"], want_sum=c["want_sum"], want_y32=c["want_y32"])
    if c["clamp"] > 0:
        kw["clamp"] = c["clamp"]
    ref = _tup(emu.layer_norm(c["x"], c["w"], c["b"], 1e-5, **kw))
    kw["residual"] = put(c["res"])
    with _selected(ops, c.get("sel")):
        got = _tup(ops.layer_norm(put(c["x"]), put(c["w"]), put(c["b"]), 1e-5, **kw))
    assert len(ref) == len(got)
    for i, (r, o) in enumerate(zip(ref, got)):
        assert r.dtype == o.dtype, (c["what"], i, r.dtype, o.dtype)
        _close(o.cpu(), r, f"{c['what']} out {i}", c["tol"])


def _vl_views(pr, Hh):
    kf = pr[..., :Hh * 256].unflatten(-1, (Hh, 256)).permute(0, 2, 1, 3)
    vo = pr[..., Hh * 256:2 * Hh * 256].unflatten(-1, (Hh, 256)).permute(0, 2, 1, 3)
    assert not kf.is_contiguous()
    return kf, vo


def _run_vlfuse(ops, emu, c, put):
    v_ln, kf, vo, bias, ob, kv, ns = c["v_ln"], c["kf"], c["vo"], c["bias"], c["ob"], c["kv"], c["ns"]
    B, Hh, T, _ = kf.shape
    if c["strided"]:                                 # the pipeline's operands: views of ONE projection output [B, T, heads*256 | heads*256 | 16]
        pr = torch.zeros(B, T, 2 * Hh * 256 + 16, dtype=kf.dtype)
        pr[..., :Hh * 256] = kf.permute(0, 2, 1, 3).reshape(B, T, -1)
        pr[..., Hh * 256:2 * Hh * 256] = vo.permute(0, 2, 1, 3).reshape(B, T, -1)
        dkf, dvo = _vl_views(put(pr), Hh)
    else:
        dkf, dvo = put(kf), put(vo)
    dv_ln, dkv = put(v_ln), put(kv)
    if "i2t" in c.get("parts", ("i2t", "t2i")):
        ref = emu.vlfuse_i2t(v_ln.float(), kf.float(), vo.float(), bias, ob.float(), kv, 0)
        got = ops.vlfuse_i2t(dv_ln, dkf, dvo, put(bias), put(ob), dkv, max_kv=0 if kv is None else int(kv.max())).cpu()
        _close(got, ref, c["what"] + ": i2t", c["tol"])
    if "t2i" in c.get("parts", ("i2t", "t2i")):
        km = None if c.get("mask") is None else ops.image_key_mask(c["mask"])
        ref = emu.vlfuse_t2i(kf.float(), v_ln.float(), ns, kv_len=kv, key_mask=km)
        got = ops.vlfuse_t2i(dkf, dv_ln, ns, kv_len=dkv, key_mask=put(km)).cpu()
        live = torch.ones(B, T, dtype=torch.bool)
        if kv is not None:                                            # rows of all-padding 128-row tiles come back as zeros by contract
            for b in range(B):
                live[b, -(-int(kv[b]) // 128) * 128:] = False
        _close(got[live], ref[live], c["what"] + ": t2i", c["tol"])


def _run_conv_dcn(ops, emu, c, put):
    x, w27, b27 = c["x"], c["w27"], c["b27"]
    dx = put(x)
    _close(ops.conv3x3_nchw32(dx, put(w27), put(b27), 27).cpu(), emu.conv3x3_nchw32(x, w27, b27, 27), c["what"] + ": offset conv", c["tol"])
    if not c["dcn"]:
        return
    w, bias, stride, om = c["w"], c["bias"], c["stride"], c["om"]
    dw, db = put(w), put(bias)
    _close(ops.conv3x3(dx, dw, db, 256, stride).cpu(), emu.conv3x3(x, w, bias, 256, stride), c["what"] + ": conv3x3", c["tol_conv"])
    y, hw = ops.dcnv2(dx, put(om), dw, db, stride)
    yr, hwr = emu.dcnv2(x, om, w, bias, stride)
    assert tuple(hw) == tuple(hwr)
    _close(y.cpu(), yr, c["what"] + ": dcnv2", c["tol_dcn"])


def _run_align_scores(ops, emu, c, put):
    dot, tb, tok, ctr = c["dot"], c["tb"], c["tok"], c["ctr"]
    d = [put(t) for t in (dot, tb, tok, ctr)]
    for agg in (0, 1, 2):
        r, cl = ops.align_scores(*d, 0.05, want_cls=True, agg=agg)
        rr, cr = emu.align_scores(dot, tb, tok, ctr, 0.05, want_cls=True, agg=agg)
        r, cl = r.cpu(), cl.cpu()
        _close(cl, cr, f"{c['what']} agg={agg}: cls", c["ftol"])
        far = (cr - 0.05).abs() > 1e-5
        _close(r[far], rr[far], f"{c['what']} agg={agg}: ranked", c["ftol"])


def _run_ml_nms(ops, emu, c, put):
    boxes, labels, nvalid, K = c["boxes"], c["labels"], c["nvalid"], c["K"]
    d = [put(t) for t in (boxes, labels, nvalid)]
    with _selected(ops, {"NMS_EARLY_STOP": 0}):
        keep = ops.ml_nms(*d, NMS_THRESH).cpu()
    ref = emu.ml_nms(boxes, labels, nvalid, NMS_THRESH)
    assert torch.equal(keep, ref), c["what"] + ": keep set"
    with _selected(ops, {"NMS_EARLY_STOP": 1}):
        part = ops.ml_nms(*d, NMS_THRESH, max_keep=K).cpu()
    for b in range(boxes.shape[0]):
        kf, kp = keep[b].nonzero().flatten(), part[b].nonzero().flatten()
        m = min(K, len(kf))
        assert torch.equal(kp[:m], kf[:m]) and bool((part[b] <= keep[b]).all()), c["what"] + ": early stop"


def _run_gcp_sparse(ops, emu, c, put):
    _close(ops.gcp_sparse_attention(put(c["q"]), put(c["kv"]), put(c["idx"])).cpu(), emu.gcp_sparse_attention(c["q"], c["kv"], c["idx"]), c["what"], c["tol"])


def _run_window_attention(ops, emu, c, put):
    a = (c["heads"], c["ws"], c["shift"])
    _close(ops.window_attention(put(c["qkv"]), put(c["qb"]), put(c["rel"]), *a).cpu(), emu.window_attention(c["qkv"], c["qb"], c["rel"], *a), c["what"], c["tol"])


def _run_window_attention_qkv(ops, emu, c, put):
    a = (c["heads"], c["ws"], c["shift"])
    _close(ops.window_attention_qkv(put(c["x"]), put(c["w"]), put(c["bias"]), put(c["rel"]), *a).cpu(),
           emu.window_attention_qkv(c["x"], c["w"], c["bias"], c["rel"], *a), c["what"], c["tol"])


def _run_dyrelu_layer_norm(ops, emu, c, put):
    N = sum(h * w for h, w in c["sizes"])
    x, dx = c["big"][:, 2:2 + N], put(c["big"])[:, 2:2 + N]
    _close(ops.dyrelu_layer_norm(dx, put(c["coef"]), c["sizes"], put(c["gam"]), put(c["bet"]), 1e-5).cpu(),
           emu.dyrelu_layer_norm(x, c["coef"], c["sizes"], c["gam"], c["bet"], 1e-5), c["what"], c["tol"])


def _run_swin_mlp2(ops, emu, c, put):
    w1f, w2f = ops.swin_mlp2_pack(c["w1"], c["w2"])
    nln = c["nln"]
    a = (c["lg"], c["lb"], 1e-5, w1f, c["b1"], w2f, c["b2"])
    got = ops.swin_mlp2(put(c["x"]), put(c["delta"]), *(put(t) if torch.is_tensor(t) else t for t in a),
                        next_ln=None if nln is None else (put(nln[0]), put(nln[1]), nln[2]), flags=c["flags"])
    ref = emu.swin_mlp2(c["x"], c["delta"], *a, next_ln=nln)
    for a_, b_, what, tol in zip(_tup(got), _tup(ref), ("out", "next LN"), (c["tol"], c["tol_next"])):
        _close(a_.cpu(), b_, f"{c['what']}: {what}", tol)


def _run_attention_text(ops, emu, c, put):
    got = ops.attention_text(put(c["qkv"]), c["H"], key_bias=put(c["kb"]), clamp=c["clamp"], kv_len=put(c["kl"]) if c["use_kl"] else None, max_kv=c["mk"])
    _close(got.cpu(), emu.attention_text(c["qkv"], c["H"], key_bias=c["kb"], clamp=c["clamp"]), c["what"], c["tol"])


def _run_patch_embed(ops, emu, c, put):
    img, w, prm = c["img"], c["w"], c["prm"]
    if c["nchw"]:
        pix, wpk = img.float().contiguous(), ops.patch_embed_pack(w.float(), nchw=True).to(w.dtype)
    else:
        pix, wpk = img.permute(0, 2, 3, 1).contiguous(), ops.patch_embed_pack(w.float()).to(w.dtype)
    rpix, rwpk = pix, wpk
    if pix.dtype == torch.float32 and not c["nchw"]:          # precise mode: channels-last FLOAT pixels; the restatement reads float pixels as NCHW
        rpix, rwpk = pix.permute(0, 3, 1, 2).contiguous(), ops.patch_embed_pack(w.float(), nchw=True)
    for a_, b_, what in zip(ops.patch_embed(put(pix), put(wpk), *(put(p) for p in prm)), emu.patch_embed(rpix, rwpk, *prm), ("stream", "norm1")):
        _close(a_.cpu(), b_, f"{c['what']}: {what}", c["tol"])


def _run_post(ops, emu, c, put):
    ranked, reg, anchors, ks, lab, wh, what = c["ranked"], c["reg"], c["anchors"], c["ks"], c["lab"], c["wh"], c["what"]
    assert ops.post_select_supported([h * w_ for h, w_ in c["shapes"]], ks, c["B"], c["L"])
    gb, gs, gl, gi = ops.post_select([put(t) for t in ranked], [put(t) for t in reg], [put(t) for t in anchors], ks, put(lab), put(wh))
    eb, es, el, ei = emu.post_select(ranked, reg, anchors, ks, lab.long(), wh)
    assert torch.equal(gi.cpu(), ei) and torch.equal(gl.cpu().int(), el.int()), what + ": candidate ids / labels"
    _close(gs.cpu(), es, what + ": scores", 2e-7)
    _close(gb.cpu(), eb, what + ": boxes", 1e-6)
    hb, hs, hl, hn = ops.post_sort(gb, gs, gl, ks)
    sb, ss, sl, sn = emu.post_sort(gb.cpu(), gs.cpu(), gl.cpu(), ks)
    assert (torch.equal(hs.cpu(), ss) and torch.equal(hl.cpu().int(), sl.int()) and torch.equal(hn.cpu().int(), sn.int())
            and torch.equal(hb.cpu(), sb)), what + ": merge"
    ho, hc = ops.post_finalize(hb, hs, hl, put(c["keep"]), c["K"], c["K2"])
    fo, fc = emu.post_finalize(hb.cpu(), hs.cpu(), hl.cpu(), c["keep"], c["K"], c["K2"])
    assert torch.equal(hc.cpu().int(), fc.int()) and torch.equal(ho.cpu(), fo), what + ": finalize"


def _run_conv_group(ops, emu, c, put):
    tok, w, bias, sizes = c["tok"], c["w"], c["bias"], c["sizes"]
    B = tok.shape[0]
    wp = torch.cat([w.permute(0, 2, 3, 1).reshape(27, -1), torch.zeros(5, 9 * 256, dtype=w.dtype)], 0).contiguous()
    dtok, dwp, dbias = put(tok), put(wp), put(bias)
    lv, dlv, off = [], [], 3
    for (h, w_) in sizes:
        lv.append(tok[:, off:off + h * w_].reshape(B, h, w_, 256))
        dlv.append(dtok[:, off:off + h * w_].reshape(B, h, w_, 256))
        off += h * w_
    got = ops.conv3x3_nchw32_group(dlv, dwp, dbias, 27)
    for l, (x, dx, y) in enumerate(zip(lv, dlv, got)):
        what = f"{c['what']} level {l}"
        _close(y.cpu(), ops.conv3x3_nchw32(dx, dwp, dbias, 27).cpu(), what + " vs the per-level kernel", c["ftol_level"])
        _close(y.cpu(), F.conv2d(x.float().permute(0, 3, 1, 2), w.float(), bias.float(), padding=1), what + " vs F.conv2d", c["ftol"])


def _run_epilogue_group(ops, emu, c, put):
    B, sizes = c["B"], c["sizes"]
    w0, b0, w2, b2 = (put(c[k]) for k in ("w0", "b0", "w2", "b2"))
    out_g = put(torch.zeros(B, sum(h * w_ for h, w_ in sizes), 256, dtype=c["w0"].dtype))
    out_p = torch.zeros_like(out_g)
    levels, off = [], 0
    for (h, w_), brs in zip(sizes, c["levels"]):
        levels.append(([(put(t), put(s), bh, bw) for t, s, bh, bw in brs], h, w_, off))
        off += h * w_
    rc = put(torch.zeros(len(sizes), B, 4, 256))
    ops.dyconv_epilogue_group([(br, h, w_, out_g[:, o:o + h * w_]) for br, h, w_, o in levels], w0, b0, w2, b2, rc)
    for l, (br, h, w_, o) in enumerate(levels):
        _, pool = ops.dyconv_fuse(br, h, w_, out=out_p[:, o:o + h * w_])
        ref = ops.dyrelu_coef(pool, h * w_, w0, b0, w2, b2)
        assert torch.equal(rc[l], ref), f"{c['what']} level {l}: DYReLU coefficients"
    assert torch.equal(out_g, out_p), c["what"]


def _run_roi_align(ops, emu, c, put):
    feat, rois = c["feat"], c["rois"]
    f16 = feat.to(c.get("h16", torch.float16)).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)                 # NHWC memory, NCHW view
    df16 = put(f16.permute(0, 2, 3, 1).contiguous()).permute(0, 3, 1, 2)
    for aligned, sr in zip((False, True), c["srs"]):
        for f, df in ((f16, df16), (feat, put(feat))):
            if f.dtype == torch.bfloat16:
                continue                                   # (ROIAlign takes fp16 / fp32 features)
            _close(ops.roi_align(df, put(rois), 7, 1.0 / 16, sr, aligned=aligned).cpu(), emu.roi_align(f, rois, 7, 1.0 / 16, sr, aligned=aligned),
                   f"{c['what']} aligned={aligned} sr={sr} {f.dtype}", c["ftol"])


def _run_msda_q(ops, emu, c, put):
    _close(ops.ms_deform_attn_q(put(c["value"]), c["shapes"], put(c["qp"]), put(c["ref_pts"]), c["M"], valid_hw=put(c["vhw"])).cpu(),
           emu.ms_deform_attn_q(c["value"], c["shapes"], c["qp"], c["ref_pts"], c["M"], valid_hw=c["vhw"]), c["what"], c["tol"])


def _run_clamp_gelu_clamp(ops, emu, c, put):
    _close(ops.clamp_gelu_clamp(put(c["x"]), c["clamp"]).cpu(), emu.clamp_gelu_clamp(c["x"], c["clamp"]), c["what"], c["tol"])


def _run_patch_merge_ln(ops, emu, c, put):
    _close(ops.patch_merge_ln(put(c["x"]), put(c["w"]), put(c["b"]), 1e-5).cpu(), emu.patch_merge_ln(c["x"], c["w"], c["b"], 1e-5), c["what"], c["tol"])


def _run_pool2x2_tokens(ops, emu, c, put):
    feats = [f.permute(0, 3, 1, 2) for f in c["feats"]]                  # NHWC memory, NCHW views: what the FPN hands over
    dfeats = [put(f).permute(0, 3, 1, 2) for f in c["feats"]]
    assert ops.pool2x2_tokens_supported(dfeats), c["what"]
    got, ref = ops.pool2x2_tokens(dfeats).cpu(), emu.pool2x2_tokens(feats)
    assert got.shape == ref.shape and torch.equal(got, ref), f"{c['what']}: max |err| {float((got.float() - ref.float()).abs().max()):.3e}"


def _run_add_upsample(ops, emu, c, put):
    ref = emu.add_upsample_nearest_(c["dst"].clone(), c["src"])
    got = ops.add_upsample_nearest_(put(c["dst"].clone()), put(c["src"]))
    _close(got.cpu(), ref, c["what"], c["tol"])


def _run_dyrelu_apply(ops, emu, c, put):
    ref = emu.dyrelu_apply_(c["x"].clone(), c["coef"])
    got = ops.dyrelu_apply_(put(c["x"].clone()), put(c["coef"]))
    _close(got.cpu(), ref, c["what"], c["tol"])


def _run_box_decode(ops, emu, c, put):
    B, tot, K = c["val"].shape[0], c["tot"], c["val"].shape[1]
    outs = []
    for o, p in ((emu, lambda t: t), (ops, put)):
        boxes, scores, labels = p(torch.full((B, tot, 4), -7.0)), p(torch.full((B, tot), -7.0)), p(torch.full((B, tot), -7, dtype=torch.int32))
        o.box_decode(p(c["val"]), p(c["flat"]), p(c["reg"]), p(c["anchors"]), p(c["lab"]), p(c["wh"]), boxes, scores, labels, c["HW"], c["L"], c["off"])
        outs.append((boxes.cpu(), scores.cpu(), labels.cpu()))
    (rb, rs, rl), (gb, gs, gl) = outs
    assert torch.equal(gl, rl), c["what"] + ": labels (and the slots outside [off, off + K) untouched)"
    _close(gs, rs, c["what"] + ": scores", c["ftol_score"])
    _close(gb, rb, c["what"] + ": boxes", c["ftol"])
    sl = slice(c["off"], c["off"] + K)
    keep = torch.ones(tot, dtype=torch.bool)
    keep[sl] = False
    assert torch.equal(gb[:, keep], rb[:, keep]) and torch.equal(gs[:, keep], rs[:, keep]), c["what"] + ": rows outside the slice were written"


def _run_bert_qkv(ops, emu, c, put):
    C, H = BERT_C, BERT_HEADS
    x, dx = c["xs"][:, :, :C], put(c["xs"])[:, :, :C]                      # row stride C + 8: a view, as the LayerNorm kernel may hand it over
    B, T = x.shape[:2]                                                     # emu.bert_attention_qkv, for any T (V^T padded to 8 keys as ops.attention wants it)
    q, k, v = F.linear(x.float(), c["w"].float(), c["bq"].float()).to(x.dtype).split(C, -1)
    vt = F.pad(v, (0, 0, 0, (-T) % 8)).transpose(1, 2).contiguous()
    ref = emu.attention4(q.reshape(B, T, H, -1), k.reshape(B, T, H, -1), vt.view(B, H, C // H, -1), c["kb"], None, c["clamp"], nk=T)
    w = ops.pack_b_fragments(c["w"]) if c["packed"] else c["w"]
    got = ops.bert_attention_qkv(dx, put(w), put(c["bq"]), H, key_bias=put(c["kb"]), clamp=c["clamp"], kv_len=put(c["kl"]) if c["use_kl"] else None,
                                 packed=c["packed"])
    _close(got.cpu(), ref, c["what"], c["tol"])


def _run_gcp_attention(ops, emu, c, put):
    x, kv, idx, lns = c["x"], c["kv"], c["idx"], c["lns"]
    ws = [c[k] for k in ("wq", "wout", "wg1")]
    ref = emu.gcp_attention(x, kv, idx, *ws, c["w2"], lns[0], lns[1], lns[2] if c["lnf"] else None, want_gate=True)
    rb = 16 if (ops.f32_operands() and c["rb"] == 32) else c["rb"]         # the fp32-operand build holds 16 rows per workgroup
    dws = [put(ops.pack_b_fragments(w)) if c["packed"] else put(w) for w in ws]
    dl = [tuple(put(t) for t in ln) for ln in lns]
    got = _tup(ops.gcp_attention(put(x), put(kv), put(idx), *dws, put(c["w2"]), dl[0], dl[1], dl[2] if c["lnf"] else None, want_gate=c["want_gate"],
                                 rows_per_block=rb, packed=c["packed"]))
    assert len(got) == 1 + int(c["lnf"]) + int(c["want_gate"]), c["what"]
    out = got[0].cpu()
    _close(out, ref[0], c["what"] + ": x_out (fp32 stream)", c["tol"])
    if c["lnf"]:
        _close(got[1].cpu(), ref[1], c["what"] + ": LN_f(x_out)", c["tol"])
    if c["want_gate"]:
        _close(got[-1].cpu(), ref[-1], c["what"] + ": gate", c["tol_gate"])
    dead = (idx < 0).all(-1)
    assert torch.equal(out[dead], x[dead]), c["what"] + ": rows without a vision query pass through bit for bit"


def _run_gcp_gate_residual(ops, emu, c, put):
    ref = _tup(emu.gcp_gate_residual(c["sup"], c["h"], c["w2"], c["x"], want_gate=c["want_gate"]))
    got = _tup(ops.gcp_gate_residual(put(c["sup"]), put(c["h"]), put(c["w2"]), put(c["x"]), want_gate=c["want_gate"]))
    assert got[0].dtype == c["x"].dtype
    _close(got[0].cpu(), ref[0], c["what"], c["tol"])
    if c["want_gate"]:
        _close(got[1].cpu(), ref[1], c["what"] + ": gate", c["ftol"])


def _run_align_fused(ops, emu, c, put):
    names = ("tok", "tk", "tbias", "wbc", "bbc", "scales", "tokidx")
    kw = dict(agg=c["agg"], kv_max=c["kv_max"], want_cls=True, want_logits=True)
    ref = emu.align_fused(*(c[k] for k in names), c["sizes"], 0.05, **kw)
    got = ops.align_fused(*(put(c[k]) for k in names), c["sizes"], 0.05, **kw)
    T, what = c["tk"].shape[1], c["what"]
    live = c["kv_max"] if 0 < c["kv_max"] < T else T
    nvb = min(T, -(-live // 16) * 16)                                      # columns beyond the live 16-token blocks are zero by contract
    _close(got["logits"].cpu()[:, :, :nvb], ref["logits"][:, :, :nvb], what + ": logits (live text blocks)", c["tol"])
    assert not bool(got["logits"].cpu()[:, :, nvb:].any()), what + ": logits beyond the live text blocks"
    _close(got["ctr"].cpu(), ref["ctr"], what + ": centerness logits", c["tol"])
    for l in range(len(c["sizes"])):
        _close(got["reg"][l].cpu(), ref["reg"][l], f"{what}: level {l} box deltas", c["tol_reg"])
        _close(got["cls"][l].cpu(), ref["cls"][l], f"{what}: level {l} class scores", c["tol"])
        far = (ref["cls"][l] - 0.05).abs() > c["tol"]                      # a score ON the threshold may fall either way
        _close(got["ranked"][l].cpu()[far], ref["ranked"][l][far], f"{what}: level {l} ranked scores", c["tol"])


def _dcn_put(br, put):
    return {k: (put(v) if torch.is_tensor(v) else v) for k, v in br.items()}


def _dcn_own_sums(y, br):
    """the statistics of the epilogue, over the kernel's own 16-bit output: (sum, sum of squares, weighted sum) per channel"""
    yf = y.float()
    n = yf.shape[1]
    wpos = torch.full((n,), 1.0 / n) if br["wy"] is None else (br["wy"][:, None] * br["wx"][None, :]).reshape(-1)
    return torch.stack([yf.sum(1), (yf * yf).sum(1), (yf * wpos[None, :, None]).sum(1)], -1)


def _run_dcn_stats(ops, emu, c, put):
    br, d = c["br"], _dcn_put(c["br"], put)
    y, hw, sums = ops.dcnv2(d["x"], d["om"], d["w"], d["bias"], d["stride"], want_stats=True, wy=d["wy"], wx=d["wx"])
    yr, hwr = emu.dcnv2(br["x"], br["om"], br["w"], br["bias"], br["stride"])
    assert tuple(hw) == tuple(hwr)
    _close(y.cpu(), yr, c["what"] + ": output", c["tol_dcn"])
    _close(sums.cpu().sum(1), _dcn_own_sums(y.cpu(), br), c["what"] + ": statistics of the kernel's own output", c["tol_stats"])
    y0, _ = ops.dcnv2(d["x"], d["om"], d["w"], d["bias"], d["stride"])
    assert torch.equal(y0.cpu(), y.cpu()), c["what"] + ": the output does not depend on want_stats"


def _run_dcn_group(ops, emu, c, put):
    ds = [_dcn_put(br, put) for br in c["brs"]]
    grouped = ops.dcnv2_group(ds)
    assert len(grouped) == len(ds)
    for i, (br, d, (yg, hwg, sg)) in enumerate(zip(c["brs"], ds, grouped)):
        what = f"{c['what']} branch {i}"
        y1, hw1, s1 = ops.dcnv2(d["x"], d["om"], d["w"], d["bias"], d["stride"], want_stats=True, wy=d["wy"], wx=d["wx"])
        assert tuple(hwg) == tuple(hw1) and torch.equal(yg.cpu(), y1.cpu()), what + ": grouped launch == single launch"
        assert torch.equal(sg.cpu(), s1.cpu()), what + ": grouped launch statistics == single launch"
        _close(yg.cpu(), emu.dcnv2(br["x"], br["om"], br["w"], br["bias"], br["stride"])[0], what + ": output", c["tol_dcn"])


RUNNERS = {"attention": _run_attention, "layer_norm": _run_layer_norm, "vlfuse": _run_vlfuse, "conv_dcn": _run_conv_dcn, "align_scores": _run_align_scores,
           "ml_nms": _run_ml_nms, "gcp_sparse": _run_gcp_sparse, "window_attention": _run_window_attention, "window_attention_qkv": _run_window_attention_qkv,
           "dyrelu_layer_norm": _run_dyrelu_layer_norm, "swin_mlp2": _run_swin_mlp2, "attention_text": _run_attention_text, "patch_embed": _run_patch_embed,
           "post": _run_post, "conv_group": _run_conv_group, "epilogue_group": _run_epilogue_group, "roi_align": _run_roi_align, "msda_q": _run_msda_q,
           "clamp_gelu_clamp": _run_clamp_gelu_clamp, "patch_merge_ln": _run_patch_merge_ln, "pool2x2_tokens": _run_pool2x2_tokens,
           "add_upsample": _run_add_upsample, "dyrelu_apply": _run_dyrelu_apply, "box_decode": _run_box_decode, "bert_qkv": _run_bert_qkv,
           "gcp_attention": _run_gcp_attention, "gcp_gate_residual": _run_gcp_gate_residual, "align_fused": _run_align_fused, "dcn_stats": _run_dcn_stats,
           "dcn_group": _run_dcn_group}


def run(ops, case, put=lambda t: t):
    import ops_emulation as emu
    safe = lambda t: None if t is None else put(t)          # noqa: E731 -- absent operands stay absent
    RUNNERS[case["op"]](ops, emu, case, safe)


# ------------------------------------------------------------------------------------------------------------------ families
class Family:
    def __init__(self, seed, base, draws, bf16=True, f32=False, exact=False):
        self.seed, self.base, self.draws = seed, base, draws        # base: cases per round (before the NMS rejection)
        self.bf16, self.f32 = bf16, f32                              # run on the device with bf16 operands / in the precise mode too
        self.exact = exact


FAMILIES = {
    "attention": Family(101, 14, draws_attention, f32=True),
    "layernorm": Family(202, 16, draws_layernorm, f32=True),
    "vlfuse": Family(303, 6, draws_vlfuse, f32=True),
    "conv_dcn": Family(404, 5, draws_conv_dcn, f32=True),
    "scoring_nms": Family(505, 12, draws_scoring_nms),
    "sparse_window": Family(606, 9, draws_sparse_window, f32=True),
    "round3_fused": Family(909, 16, draws_round3_fused, f32=True),
    "round4": Family(4004, 19, draws_round4, f32=True),
    "grouped_dyconv": Family(5005, 6, draws_grouped_dyconv, f32=True),          # (precise mode: `served` leaves the group conv out, the epilogue group runs)
    "swin_roi_msda": Family(707, 11, draws_swin_roi_msda, f32=True),
    "bf16_twins": Family(808, 20, draws_bf16_twins, bf16=False),
    "clamped": Family(1111, 12, draws_clamped, f32=True),
    "patch_merge": Family(1212, 6, draws_patch_merge, f32=True),
    "pyramid_elementwise": Family(1313, 16, draws_pyramid_elementwise),
    "vlfuse_masked": Family(1414, 4, draws_vlfuse_masked, f32=True),
    "bert_qkv": Family(1515, 3, draws_bert_qkv, f32=True),
    "gcp_fused": Family(1616, 4, draws_gcp_fused, f32=True),
    "align_fused": Family(1717, 4, draws_align_fused, f32=True),
    "dcn_stats_group": Family(1818, 4, draws_dcn_stats_group, f32=True),
}


def cases(name, n, chip=None, seed=0, **opt):
    """draws 0 .. of family `name`: n rounds (see the module docstring)"""
    fam = FAMILIES[name]
    rng = random.Random(fam.seed + seed)
    g = torch.Generator().manual_seed(fam.seed + seed)
    return fam.draws(rng, g, n, dict(EMU_CHIP) if chip is None else chip, **opt)


def _map_tensors(v, fn):
    if torch.is_tensor(v):
        return fn(v)
    if isinstance(v, (list, tuple)):
        return type(v)(_map_tensors(x, fn) for x in v)
    if isinstance(v, dict):
        return {k: _map_tensors(x, fn) for k, x in v.items()}
    return v


def _off_grid(t):
    """fp16 values as floats, moved off the fp16 grid by up to 3 / 2^14 relative (deterministic): the low halves of the split operands of the
    precise mode are then not zero.  Zeros stay zeros."""
    f = t.float()
    k = (torch.arange(f.numel(), dtype=torch.float32) % 7 - 3).reshape(f.shape)
    return f * (1.0 + k * 2.0 ** -14)


def cast_case(case, mode):
    """the case in operand mode `mode` (module docstring): "fp16" unchanged, "bf16", "f32\""""
    if mode == "fp16":
        return case
    from parity_checks import F32_TOL
    fn = (lambda t: t.to(torch.bfloat16) if t.dtype == torch.float16 else t) if mode == "bf16" else (lambda t: _off_grid(t) if t.dtype == torch.float16 else t)
    out = {}
    for k, v in case.items():
        if k.startswith("tol"):
            out[k] = v * 8 if mode == "bf16" else min(v, F32_TOL)
        else:
            out[k] = _map_tensors(v, fn)
    out["h16"] = torch.bfloat16 if mode == "bf16" else torch.float32
    out["what"] = f"[{mode}] " + case["what"]
    return out


def served(ops, case):
    """does the product serve this case in the CURRENT operand mode?  Decided by the product's own predicates, never by trying."""
    op = case["op"]
    if op == "bert_qkv":
        return ops.bert_attention_qkv_fits(case["xs"].shape[1], BERT_C, BERT_HEADS, case["kb"])
    if op == "gcp_attention":
        return ops.gcp_attention_fits(case["x"], case["idx"])
    if op == "align_fused":
        return ops.align_fused_fits(case["tk"].shape[1], case["kv_max"])
    if op == "conv_group":                                               # (precise mode: the window of all 256 channels does not fit -- per-level kernel)
        tok, off, lv = case["tok"], 3, []
        for (h, w_) in case["sizes"]:
            lv.append(tok[:, off:off + h * w_].reshape(tok.shape[0], h, w_, 256))
            off += h * w_
        return ops.conv3x3_nchw32_group_supported(lv, 27)
    if op == "attention_text":
        return ops.attention_text_fits(case["qkv"].shape[1], case["kl"] if case["use_kl"] else None, case["mk"])
    return True


# ------------------------------------------------------------------------------------------------------------------ digests
def _feed(h, v):
    if torch.is_tensor(v):
        t = v.detach().contiguous()
        h.update(f"T{t.dtype}{tuple(t.shape)}".encode())
        h.update(t.view(torch.uint8).numpy().tobytes() if t.numel() else b"")
    elif isinstance(v, (list, tuple)):
        h.update(f"L{len(v)}".encode())
        for x in v:
            _feed(h, x)
    elif isinstance(v, dict):
        h.update(f"D{len(v)}".encode())
        for k in sorted(v):
            h.update(str(k).encode())
            _feed(h, v[k])
    elif isinstance(v, float):
        h.update(b"F" + struct.pack("<d", v))
    elif isinstance(v, bool) or v is None or isinstance(v, (int, str)):
        h.update(f"{type(v).__name__}:{v}".encode())
    else:
        raise TypeError(f"case value of type {type(v)}")


DIGEST_SKIP = ("what", "tol", "ftol", "sel")          # labels, tolerances and kernel selection are not inputs


def case_digest(h, case):
    for k in sorted(case):
        if not k.startswith(DIGEST_SKIP):
            h.update(k.encode())
            _feed(h, case[k])


def family_digest(name, n=1, seed=0, **opt):
    h = hashlib.sha256()
    for case in cases(name, n, seed=seed, **opt):
        case_digest(h, case)
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------------------------ replay
def replay_line(name, k, seed=0, device="cpu", dtype="fp16", env=None, opt=None):
    parts = [f"python tests/fuzz_cases.py {name} {k}"]
    if seed:
        parts.append(f"--seed {seed}")
    parts += [f"--device {device}", f"--dtype {dtype}"]
    if env:
        parts.append("--env " + " ".join(f"{a}={b}" for a, b in sorted(env.items())))
    if opt:
        parts.append("--opt " + " ".join(f"{a}={b}" for a, b in sorted(opt.items())))
    return " ".join(parts)


def device_chip(f32=False):
    return {"cus": torch.cuda.get_device_properties(0).multi_processor_count, "f32": bool(f32)}


def parse_opt(items):
    """--opt k=v ... : draw options of a family (conv_dcn: full=0|1)"""
    return {k: bool(int(v)) for k, v in (i.split("=", 1) for i in items or ())}


def _main(argv):
    import argparse
    ap = argparse.ArgumentParser(description="regenerate draws 0 .. k of a family and run draw k alone")
    ap.add_argument("family", choices=sorted(FAMILIES))
    ap.add_argument("draw", help="index of the draw to run, or 'all' (every draw of --rounds rounds)")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", choices=("cpu", "cuda"), default="cpu")
    ap.add_argument("--dtype", choices=("fp16", "bf16", "f32"), default="fp16")
    ap.add_argument("--env", nargs="*", default=[], metavar="MQ_X=v")
    ap.add_argument("--opt", nargs="*", default=[], metavar="k=v")
    ap.add_argument("--cus", type=int, default=0, help="compute units of the chip the draw was made for (cpu replay of a device draw of the Swin-MLP split)")
    a = ap.parse_args(argv)
    for kv in a.env:
        k, v = kv.split("=", 1)
        os.environ[k] = v
    if a.dtype == "f32":
        os.environ["MQ_F32_OPERANDS"] = "1"
    from mq_det_amd import ops
    if a.device == "cuda":
        chip = device_chip(a.dtype == "f32")
    else:
        chip = {"cus": a.cus or EMU_CHIP["cus"], "f32": a.dtype == "f32"}
    every = a.draw == "all"
    k = -1 if every else int(a.draw)
    todo = []
    for i, c in enumerate(cases(a.family, a.rounds if every else k + 1, chip, a.seed, **parse_opt(a.opt))):
        if every or i == k:
            c = cast_case(c, a.dtype)
            c["what"] = f"{a.family} draw {i}: {c['what']}"
            todo.append(c)
            if not every:
                break
    assert todo, f"family {a.family} has no draw {a.draw}"
    with contextlib.ExitStack() as st:
        if a.device == "cuda":
            ops.load_library()
            ops.configure()
            dev = torch.device("cuda:0")
            put = lambda t: t.to(dev)          # noqa: E731
        else:
            import simt
            from simt import guard
            ops = st.enter_context(simt.installed(f32=1 if a.dtype == "f32" else False))
            st.enter_context(guard.pointer_guard())
            put = lambda t: t                  # noqa: E731
        for c in todo:
            print(c["what"], flush=True)
            if not served(ops, c):
                print("  not served in this operand mode", flush=True)
                continue
            run(ops, c, put)
        if a.device == "cuda":
            torch.cuda.synchronize()
    print("draw ok")
    return 0


if __name__ == "__main__":
    sys.exit(_main(sys.argv[1:]))
