"""Times the convolutions of the FPN neck and the RPN trunk at the benchmark geometries, in one process on one GPU:

    config 2   B = 2, 64 x 64 patch grid (1024^2, ViT-B), Cin 768, Cout 256
    config 4   B = 1, 80 x 80 patch grid (1280^2, ViT-L), Cin 1024, Cout 256
    stages     the four laterals (1x1, Cin -> 256; levels 0-2 with the top-down add in the epilogue on the HIP route), the four
               output convolutions (3x3, 256 -> 256), the RPN trunk's five levels (3x3 + ReLU, 256 -> 256) and its packed
               cls | reg heads (1x1, 256 -> 16, fp32 out)
    routes     `hip` = as_conv2d_fwd (csrc/conv.hip) through ops.conv2d_nhwc; `bf16` = F.conv2d on the same device tensors, bf16
               channels-last; `fp32` = F.conv2d in fp32 (NCHW).  The F.conv2d routes time the convolution alone (no upsample + add).

Every figure is the HIP-event time of --calls back-to-back calls after a warm-up, divided by the calls; the routes alternate
inside each of --rounds rounds and the median round is reported.  FLOPs are 2 B H W Cout ksize^2 Cin from the shapes; the share
of peak is against 2.5 PFLOP/s (bf16 dense MFMA).  Prints a markdown table (profiles/neck_bench.md is this output).

    python tools/neck_bench.py [--calls 50] [--rounds 3] [--out profiles/neck_bench.md]
    python tools/neck_bench.py --dry-run          # shapes and FLOP counts, no device
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK = 2.5e15
CONFIGS = [("config 2", 2, 64, 768), ("config 4", 1, 80, 1024)]
COUT = 256


def stages(B, grid, cin):
    """-> [(name, B, H, W, Cin, Cout, ksize, act, out fp32, add (Ha, Wa) | None)]"""
    sizes = [(4 * grid, 4 * grid), (2 * grid, 2 * grid), (grid, grid), (grid // 2, grid // 2)]
    sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    out = []
    for l in range(4):
        out.append((f"lateral {l} (stride {4 << l})", B, *sizes[l], cin, COUT, 1, "none", False, sizes[l + 1] if l < 3 else None))
    for l in range(4):
        out.append((f"output {l} (stride {4 << l})", B, *sizes[l], COUT, COUT, 3, "none", False, None))
    for l in range(5):
        out.append((f"rpn trunk {l} (stride {4 << l})", B, *sizes[l], COUT, COUT, 3, "relu", False, None))
    for l in range(5):
        out.append((f"rpn heads {l} (stride {4 << l})", B, *sizes[l], COUT, 16, 1, "none", True, None))
    return out


def flops(st):
    _, B, H, W, cin, cout, k, _, _, _ = st
    return 2.0 * B * H * W * cout * k * k * cin


def events(fn, calls):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / calls


def count_launches():
    """as_conv2d_fwd launches of one FPN + RPNHead forward on the HIP route"""
    import attentionshift_amd as A
    from attentionshift_amd import ops
    neck = A.build_neck(dict(type="FPN", in_channels=[64] * 4, out_channels=32, num_outs=5)).cuda()
    rpn = A.build_head(dict(type="RPNHead", in_channels=32, feat_channels=32, compute_dtype=torch.bfloat16)).cuda()
    calls, real = [], ops.conv2d_nhwc
    ops.conv2d_nhwc = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        with torch.no_grad():
            rpn(neck([torch.randn(1, 64, 32 >> l, 32 >> l, device="cuda") for l in range(4)]))
    finally:
        ops.conv2d_nhwc = real
    return len(calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.dry_run:
        for name, B, grid, cin in CONFIGS:
            total = 0.0
            print(f"{name}: B = {B}, {grid} x {grid} patch grid, Cin {cin}, Cout {COUT}")
            for st in stages(B, grid, cin):
                total += flops(st)
                add = "" if st[9] is None else f", add from {st[9][0]} x {st[9][1]}"
                print(f"  {st[0]:<28} [{st[1]}, {st[2]}, {st[3]}, {st[4]}] -> {st[5]}, {st[6]}x{st[6]}{add}: {flops(st) / 1e9:9.3f} GFLOP")
            print(f"  total {total / 1e12:.3f} TFLOP")
        return
    assert torch.cuda.is_available(), "needs a GPU (use --dry-run for the shapes)"
    if args.calls < 50:
        raise SystemExit("--calls must be at least 50")
    from attentionshift_amd import ops
    gen = torch.Generator().manual_seed(2)
    lines = ["# FPN neck and RPN trunk: as_conv2d_fwd against torch's convolution",
             "",
             f"`python tools/neck_bench.py --calls {args.calls} --rounds {args.rounds}` on {torch.cuda.get_device_name(0)}.  HIP-event time of "
             f"{args.calls} back-to-back calls after a warm-up, per call; the three routes alternate inside each of {args.rounds} rounds, the "
             "median round is shown.  `hip` = `as_conv2d_fwd` (csrc/conv.hip); `bf16` / `fp32` = `F.conv2d` on the same device tensors "
             "(bf16 channels-last / fp32), the convolution alone.  TFLOP/s from 2 B H W Cout k^2 Cin; share of the 2.5 PFLOP/s bf16 peak.",
             ""]
    for name, B, grid, cin in CONFIGS:
        lines += [f"## {name}: B = {B}, {grid} x {grid} patch grid, Cin {cin}, Cout {COUT}", "",
                  "| stage | shape [B, H, W, Cin] -> Cout, k | GFLOP | hip ms | hip TFLOP/s | hip share of peak | bf16 ms | bf16 TFLOP/s | fp32 ms | hip / bf16 |",
                  "|---|---|---|---|---|---|---|---|---|---|"]
        tot = dict(hip=0.0, bf16=0.0, fp32=0.0, flop=0.0)
        for st in stages(B, grid, cin):
            sname, _, H, W, ci, co, k, act, f32out, add_hw = st
            w = torch.randn(co, ci, k, k, generator=gen) / (k * k * ci) ** 0.5
            x = torch.randn(B, H, W, ci, generator=gen).to(torch.bfloat16).cuda()
            bias = torch.randn(co, generator=gen).cuda()
            add = None if add_hw is None else torch.randn(B, add_hw[0], add_hw[1], co, generator=gen).to(torch.bfloat16).cuda()
            wp = ops.pack_conv_weight(w.cuda())
            x_cl = x.permute(0, 3, 1, 2)                                 # NCHW-shaped view of channels-last memory
            w_cl = w.cuda().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            b_bf = bias.to(torch.bfloat16)
            x32, w32 = x_cl.float().contiguous(), w.cuda()
            od = torch.float32 if f32out else torch.bfloat16
            relu = act == "relu"
            routes = dict(
                hip=lambda: ops.conv2d_nhwc(x, wp, bias, ksize=k, act=act, add=add, out_dtype=od),
                bf16=lambda: (F.relu_(F.conv2d(x_cl, w_cl, b_bf, padding=k // 2)) if relu else F.conv2d(x_cl, w_cl, b_bf, padding=k // 2)),
                fp32=lambda: (F.relu_(F.conv2d(x32, w32, bias, padding=k // 2)) if relu else F.conv2d(x32, w32, bias, padding=k // 2)))
            with torch.no_grad():
                got = {r: [] for r in routes}
                for _ in range(args.rounds):
                    for r, fn in routes.items():
                        got[r].append(events(fn, args.calls))
            t = {r: statistics.median(v) for r, v in got.items()}
            fl = flops(st)
            for r in t:
                tot[r] += t[r]
            tot["flop"] += fl
            print(f"[neck_bench] {name}: {sname} hip {t['hip'] * 1e3:.4f} ms, bf16 {t['bf16'] * 1e3:.4f} ms, fp32 {t['fp32'] * 1e3:.4f} ms",
                  file=sys.stderr, flush=True)
            lines.append(f"| {sname} | [{B}, {H}, {W}, {ci}] -> {co}, {k} | {fl / 1e9:.2f} | {t['hip'] * 1e3:.4f} | {fl / t['hip'] / 1e12:.1f} | "
                         f"{fl / t['hip'] / PEAK:.3f} | {t['bf16'] * 1e3:.4f} | {fl / t['bf16'] / 1e12:.1f} | {t['fp32'] * 1e3:.4f} | "
                         f"{t['hip'] / t['bf16']:.2f} |")
            del x, x_cl, x32, w32, w_cl, wp, add
            torch.cuda.empty_cache()
        lines += [f"| **sum** | | {tot['flop'] / 1e9:.1f} | {tot['hip'] * 1e3:.3f} | {tot['flop'] / tot['hip'] / 1e12:.1f} | "
                  f"{tot['flop'] / tot['hip'] / PEAK:.3f} | {tot['bf16'] * 1e3:.3f} | {tot['flop'] / tot['bf16'] / 1e12:.1f} | "
                  f"{tot['fp32'] * 1e3:.3f} | {tot['hip'] / tot['bf16']:.2f} |", ""]
    lines += [f"Launches of `as_conv2d_fwd` in one `FPN` + `RPNHead(compute_dtype=torch.bfloat16)` forward: {count_launches()} "
              "(4 laterals + 4 outputs + 2 per RPN level).", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
