"""Times the test-time post-processing of one image on both routes, in one process on one GPU:

    multiclass_nms   1000 proposals x 20 classes, score_thr 0.05, IoU 0.5, 100 kept (the shipped VOC test config)
    get_seg_masks    100 detections, 28 x 28 masks, a 1024 x 1024 image, threshold 0.5
    ... to COCO RLE  the same masks as run-length strings: get_seg_masks(encode_rle=True), encoded on the device
                     (csrc/rle.hip), against the bitmap get_seg_masks + encode_mask_results on the host; and the
                     encode kernels alone
    get_det_bboxes   the stage from the box head's outputs to the detections (softmax, decode, rescale, threshold, order, NMS) at
                     1000 x 20, 1000 x 80 and 300 x 20: the fused candidates of csrc/det.hip (fused=True) against the tensor ops
                     of the default route, both followed by as_nms; HIP events around each call, the count readbacks included
    rpn_proposals    one image's five levels at 1024 x 1024 (261 888 anchors), nms_pre 1000, max_per_img 1000, IoU 0.7 (the
                     shipped test_cfg.rpn): csrc/rpn.hip + as_nms against the tensor-op route, and the stage before NMS alone

`device` = csrc/detect_post.hip (as_nms / as_paste_masks), `host` = the tensor-op route on the same device tensors
(AS_POST_HOST=1: full IoU matrix + Python loop; sigmoid over all classes + grid_sample).  Every call is followed by a device
synchronize; the figure is the median of --repeats calls after --warmup, the two routes alternating call by call.  Prints a markdown table (profiles/post_bench.md
is this output) and checks that both routes return the same detections.

    python tools/post_bench.py [--repeats 10] [--warmup 2] [--out profiles/post_bench.md]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from attentionshift_amd import inference as I      # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s, MI355X


def _route(route):
    if route == "host":
        os.environ["AS_POST_HOST"] = "1"
    else:
        os.environ.pop("AS_POST_HOST", None)


def both_routes(fn, repeats, warmup, switch=True):
    """-> {route: (median s, min s, last result)}; the routes alternate call by call, so that a drift of the box (other
    tenants, allocator warm-up) falls on both alike.  switch=False leaves AS_POST_HOST alone: fn(route) tells the two
    apart itself."""
    ts, out = {"device": [], "host": []}, {}
    for r in range(warmup + repeats):
        for route in ("device", "host"):
            if switch:
                _route(route)
            t0 = time.perf_counter()
            out[route] = fn(route)
            torch.cuda.synchronize()
            if r >= warmup:
                ts[route].append(time.perf_counter() - t0)
    _route("device")
    return {k: (statistics.median(v), min(v), out[k]) for k, v in ts.items()}


def rle_kernels_alone(masks, repeats):
    """-> seconds per encode (as_rle_count + as_rle_encode back to back) between HIP events: no readback, no allocation"""
    from attentionshift_amd import _lib
    lib = _lib.load()
    n, H, W = masks.shape
    nbytes = lib.as_rle_workspace_bytes(n, H, W)
    ws = torch.empty(nbytes, device=masks.device, dtype=torch.uint8)
    totals = torch.empty(n, device=masks.device, dtype=torch.int32)
    st = torch.cuda.current_stream().cuda_stream

    def count():
        _lib.check(lib.as_rle_count(masks.data_ptr(), n, H, W, totals.data_ptr(), ws.data_ptr(), nbytes, st), "as_rle_count")
    count()
    runs = int(totals.sum())
    pos = torch.empty(max(runs, 1), device=masks.device, dtype=torch.int32)
    out = torch.empty(8 * n + 7 * (runs + n), device=masks.device, dtype=torch.uint8)

    def encode():
        _lib.check(lib.as_rle_encode(masks.data_ptr(), n, H, W, totals.data_ptr(), ws.data_ptr(), nbytes, pos.data_ptr(), runs,
                                     out.data_ptr() + 8 * n, 7 * (runs + n), out.data_ptr(), st), "as_rle_encode")
    encode()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(repeats):
        count()
        encode()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / repeats, runs, out.numel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--legs", default="all", choices=["all", "det"], help="det: only the get_det_bboxes leg")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.set_grad_enabled(False)
    if args.legs == "det":
        text = "\n".join(det_leg(args)[1:]) + "\n"
        print(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text)
        return
    gen = torch.Generator().manual_seed(2)
    n, K = 1000, 20
    xy = torch.rand(n, 2, generator=gen) * 900
    boxes = torch.cat((xy, xy + 10 + torch.rand(n, 2, generator=gen) * 200), 1)
    per_class = (boxes[:, None, :] + torch.randn(n, K, 4, generator=gen) * 4).reshape(n, 4 * K).cuda()
    scores = torch.softmax(torch.randn(n, K + 1, generator=gen) * 2.5, 1).cuda()
    candidates = int((scores[:, :-1] > 0.05).sum())
    nms = both_routes(lambda route: I.multiclass_nms(per_class, scores, 0.05, 0.5, 100), args.repeats, args.warmup)
    (dd, ld), (dh, lh) = nms["device"][2], nms["host"][2]
    assert torch.equal(ld, lh) and torch.equal(dd, dh), "the two NMS routes disagree"

    m, H, W = 100, 1024, 1024
    logits = (torch.randn(m, K, 28, 28, generator=gen) * 3).cuda()
    bxy = torch.rand(m, 2, generator=gen) * 700
    dets = torch.cat((bxy, bxy + 40 + torch.rand(m, 2, generator=gen) * 280, torch.rand(m, 1, generator=gen)), 1).cuda()
    labels = torch.randint(0, K, (m,), generator=gen).cuda()
    seg = both_routes(lambda route: I.get_seg_masks(logits, dets, labels, K, (H, W, 3), 1.0, True, 0.5), args.repeats, args.warmup)
    sd, sh = (np.stack([x for s in r[2] for x in s]) for r in (seg["device"], seg["host"]))
    differ = int((sd != sh).sum())
    # the paste without the copy of the [m,H,W] bytes to the host and the per-class lists: the kernel against its floor
    from attentionshift_amd import ops
    box4 = dets[:, :4].contiguous()
    paste = both_routes(lambda route: ops.paste_masks(logits, labels, box4, H, W, True, 1, 0.5) if route == "device"
                        else _host_paste(logits, labels, box4, H, W), args.repeats, args.warmup)
    t_k, t_h = paste["device"][0], paste["host"][0]
    # ... and the kernel by itself: HIP events around back-to-back launches (no launch gap, no synchronize in the figure)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.repeats):
        ops.paste_masks(logits, labels, box4, H, W, True, 1, 0.5)
    e1.record()
    torch.cuda.synchronize()
    t_ev = e0.elapsed_time(e1) * 1e-3 / args.repeats
    # the masks as COCO RLE: encoded on the device (only the strings leave it) against the bitmaps copied out and encoded
    # on the host -- both start from the same paste kernel, so the strings must be equal
    seg_args = (logits, dets, labels, K, (H, W, 3), 1.0, True, 0.5)
    rle = both_routes(lambda route: I.get_seg_masks(*seg_args, encode_rle=True) if route == "device"
                      else I.encode_mask_results(I.get_seg_masks(*seg_args)), args.repeats, args.warmup, switch=False)
    assert rle["device"][2] == rle["host"][2], "the device and the host encoding disagree"
    rle_bytes = sum(len(r["counts"]) for c in rle["device"][2] for r in c)
    pasted = ops.paste_masks(logits, labels, box4, H, W, True, 1, 0.5)
    t_rle, runs, copied = rle_kernels_alone(pasted, args.repeats)
    assert seg["device"][0] > rle["device"][0], "encoding on the device is slower than copying the bitmaps out"

    rpn_lines = rpn_leg(args, gen)

    lines = [
        "# Test-time post-processing: device kernels against the tensor-op route",
        "",
        f"`python tools/post_bench.py --repeats {args.repeats} --warmup {args.warmup}` on {torch.cuda.get_device_name(0)}; "
        "wall time per call including the device synchronize, median (min) in ms.",
        "",
        "| stage | size | device (`csrc/detect_post.hip`) | host route (`AS_POST_HOST=1`) | host / device |",
        "|---|---|---|---|---|",
        f"| `multiclass_nms` | {n} proposals x {K} classes -> {candidates} candidates, 100 kept | "
        f"{nms['device'][0] * 1e3:.3f} ({nms['device'][1] * 1e3:.3f}) | {nms['host'][0] * 1e3:.3f} ({nms['host'][1] * 1e3:.3f}) | "
        f"{nms['host'][0] / nms['device'][0]:.1f} |",
        f"| `get_seg_masks` (to numpy lists) | {m} x 28 x 28 -> {H} x {W} | "
        f"{seg['device'][0] * 1e3:.3f} ({seg['device'][1] * 1e3:.3f}) | {seg['host'][0] * 1e3:.3f} ({seg['host'][1] * 1e3:.3f}) | "
        f"{seg['host'][0] / seg['device'][0]:.1f} |",
        f"| paste alone (result left on the device) | same | {t_k * 1e3:.3f} | {t_h * 1e3:.3f} | {t_h / t_k:.1f} |",
        "",
        f"Paste kernel: {m * H * W / 1e6:.1f} MB written in {t_k * 1e3:.3f} ms = {m * H * W / t_k / 1e12:.2f} TB/s = "
        f"{100 * m * H * W / t_k / HBM_PEAK:.1f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak (launch and synchronize included); "
        f"{t_ev * 1e3:.3f} ms per launch between HIP events over {args.repeats} back-to-back launches = "
        f"{m * H * W / t_ev / 1e12:.2f} TB/s = {100 * m * H * W / t_ev / HBM_PEAK:.1f} % of peak.",
        f"Both NMS routes return identical detections; the mask routes differ on {differ} of {sd.size} pixels.",
        "",
        "## The masks as COCO RLE (`csrc/rle.hip`)",
        "",
        "Both columns paste on the device; they alternate call by call like the routes above.",
        "",
        "| stage | encoded on the device: `get_seg_masks(encode_rle=True)` | bitmap `get_seg_masks` + `encode_mask_results` on the host |",
        "|---|---|---|",
        f"| {m} masks {H} x {W} to per-class lists of RLE dicts | {rle['device'][0] * 1e3:.3f} ({rle['device'][1] * 1e3:.3f}) | "
        f"{rle['host'][0] * 1e3:.3f} ({rle['host'][1] * 1e3:.3f}) |",
        "",
        f"Bitmap `get_seg_masks` alone (the device column of the first table, no encoding at all): {seg['device'][0] * 1e3:.3f} ms; "
        f"with the encoding on the device: {rle['device'][0] * 1e3:.3f} ms = {seg['device'][0] / rle['device'][0]:.1f} x faster, "
        f"{rle['host'][0] / rle['device'][0]:.0f} x faster than copying out and encoding on the host.",
        f"Encode kernels (`as_rle_count` + `as_rle_encode`, five launches): {t_rle * 1e3:.3f} ms between HIP events over "
        f"{args.repeats} back-to-back encodes; they read the masks twice, {2 * m * H * W / 1e6:.1f} MB = "
        f"{2 * m * H * W / t_rle / 1e12:.2f} TB/s = {100 * 2 * m * H * W / t_rle / HBM_PEAK:.1f} % of the HBM peak "
        "(the 105 MB fit the Infinity Cache).  "
        f"{runs} value changes in all; {copied} bytes are copied to the host ({rle_bytes} bytes of strings) instead of {m * H * W}.",
        "The device and the host encoding return identical strings.",
    ] + rpn_lines + det_leg(args)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


def _library_launches(fn):
    """-> kernel launches of the library in one call of fn: as_rpn_candidates is three, as_nms two (csrc/rpn.hip,
    csrc/detect_post.hip); counted through the wrappers that make them"""
    from attentionshift_amd import ops
    n = {"rpn": 0, "nms": 0}
    real_rpn, real_nms = ops.rpn_candidates, ops.nms
    ops.rpn_candidates = lambda *a, **k: (n.__setitem__("rpn", n["rpn"] + 1), real_rpn(*a, **k))[1]
    ops.nms = lambda *a, **k: (n.__setitem__("nms", n["nms"] + 1), real_nms(*a, **k))[1]
    try:
        fn()
    finally:
        ops.rpn_candidates, ops.nms = real_rpn, real_nms
    return 3 * n["rpn"] + 2 * n["nms"]


def rpn_leg(args, gen):
    """RPN proposals of one image at 1024 x 1024: five levels (256^2 ... 16^2 positions x 3 anchors = 261 888 anchors), the
    shipped test_cfg.rpn (nms_pre 1000, max_per_img 1000, IoU 0.7), both routes on device tensors."""
    from attentionshift_amd import ops
    from attentionshift_amd.rpn import AnchorGenerator
    ag = AnchorGenerator([8], [0.5, 1.0, 2.0], [4, 8, 16, 32, 64])
    sizes = [1024 // s for s in (4, 8, 16, 32, 64)]
    cls = [(torch.randn(1, 3, s, s, generator=gen) * 2).cuda() for s in sizes]
    reg = [(torch.randn(1, 12, s, s, generator=gen) * 0.2).cuda() for s in sizes]
    base, shapes = torch.stack(ag.base_anchors).cuda(), [(1024, 1024, 3)]
    call = lambda route: I.rpn_proposals(cls, reg, base, ag.strides, shapes, 1000, 1000, 0.7)      # noqa: E731
    res = both_routes(call, args.repeats, args.warmup)
    pd, ph = res["device"][2][0], res["host"][2][0]
    same = pd.shape == ph.shape and torch.allclose(pd, ph, rtol=1e-6, atol=1e-5)
    cand = lambda route: I.rpn_candidates(cls, reg, base, ag.strides, shapes, 1000)                # noqa: E731
    sel = both_routes(cand, args.repeats, args.warmup)
    order_equal = torch.equal(sel["device"][2][3], sel["host"][2][3]) and torch.equal(sel["device"][2][4], sel["host"][2][4])
    C = sel["device"][2][2].shape[1]
    # the three kernels of as_rpn_candidates by themselves: HIP events around back-to-back calls (allocations included)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.repeats):
        ops.rpn_candidates(cls, reg, base, ag.strides, shapes, 1000)
    e1.record()
    torch.cuda.synchronize()
    t_ev = e0.elapsed_time(e1) * 1e-3 / args.repeats
    kernels = _library_launches(lambda: call("device"))
    logit_bytes = sum(c.numel() for c in cls) * 4
    return [
        "",
        "## RPN proposals (`csrc/rpn.hip` + `as_nms`)",
        "",
        f"One image, five levels {' / '.join(f'{s}^2' for s in sizes)} x 3 anchors = {sum(3 * s * s for s in sizes)} anchors, "
        f"`nms_pre` 1000, `max_per_img` 1000, IoU 0.7 -> {C} candidates, {pd.shape[0]} proposals; inputs on the device on both "
        "routes, median (min) in ms.",
        "",
        "| stage | device (`csrc/rpn.hip`) | host route (`AS_POST_HOST=1`) | host / device |",
        "|---|---|---|---|",
        f"| `rpn_proposals` (selection, decode, level NMS, gather) | {res['device'][0] * 1e3:.3f} ({res['device'][1] * 1e3:.3f}) | "
        f"{res['host'][0] * 1e3:.3f} ({res['host'][1] * 1e3:.3f}) | {res['host'][0] / res['device'][0]:.1f} |",
        f"| `rpn_candidates` (everything before NMS) | {sel['device'][0] * 1e3:.3f} ({sel['device'][1] * 1e3:.3f}) | "
        f"{sel['host'][0] * 1e3:.3f} ({sel['host'][1] * 1e3:.3f}) | {sel['host'][0] / sel['device'][0]:.1f} |",
        "",
        f"`as_rpn_candidates` (three launches) between HIP events over {args.repeats} back-to-back calls: {t_ev * 1e3:.3f} ms; it reads "
        f"the {logit_bytes / 1e6:.2f} MB of logits twice.  Kernel launches per `rpn_proposals` call on the device route: "
        f"{kernels} of the library (3 for the candidates + 2 per image for `as_nms`) + torch's gather of the kept rows (two index "
        "selects and one concatenation per image).",
        f"The two routes select the same candidates in the same order: {order_equal}; their proposals agree within rtol 1e-6 / atol 1e-5 "
        f"(they differ in `exp` alone): {same}.",
    ]


def _count_syncs(fn):
    """-> host synchronizations torch makes in one call of fn (its sync debug mode warns at each)"""
    import warnings
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(x.message) for x in w)


def _count_launches(fn):
    """-> kernel launches in one call of fn as torch's profiler traces them (copies and memsets left out); None when the
    profiler gives no device activity"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]
        n = sum(1 for x in names if "memcpy" not in x.lower() and "memset" not in x.lower())
        return n or None
    except Exception:
        return None


def det_leg(args):
    """get_det_bboxes of one image: the default route on device tensors (tensor ops, then as_nms) against fused=True
    (as_det_candidates, one count readback, as_nms).  HIP events around every call, the routes alternating call by call."""
    lines = [
        "",
        "## The box head's detection stage (`csrc/det.hip` + `as_nms`)",
        "",
        f"`python tools/post_bench.py --legs det --repeats {args.repeats} --warmup {args.warmup}` on {torch.cuda.get_device_name(0)}.  "
        "`get_det_bboxes` of one image from the box head's outputs to the detections: logits `[n, K+1]`, per-class deltas "
        "`[n, 4K]`, a 1024 x 1024 image, rescale by four factors, `score_thr` 0.05, IoU 0.5, 100 kept.  Time between HIP events "
        "around each call, the count readbacks included, median (min) in ms; the two routes alternate call by call.  Launches are "
        "what torch's profiler traces in one call (copies and memsets left out), syncs what its sync debug mode reports.",
        "",
        "| n x K | candidates | tensor ops + `as_nms` (default) | launches | syncs | fused (`fused_det`) | launches | syncs | default / fused |",
        "|---|---|---|---|---|---|---|---|---|",
    ]
    notes, alone = [], []
    for n, K in ((1000, 20), (1000, 80), (300, 20)):
        gen = torch.Generator().manual_seed(100 * n + K)
        xy = torch.rand(n, 2, generator=gen) * 900
        rois = torch.cat((torch.zeros(n, 1), xy, xy + 10 + torch.rand(n, 2, generator=gen) * 200), 1).cuda()
        logits = (torch.randn(n, K + 1, generator=gen) * 2.5).cuda()
        pred = (torch.randn(n, 4 * K, generator=gen) * 0.5).cuda()
        sf = np.array([1.25, 1.5, 1.25, 1.5], dtype=np.float32)
        call = {r: (lambda f=(r == "fused"): I.get_det_bboxes(rois, logits, pred, (1024, 1024, 3), sf, True, 0.05, 0.5, 100, fused=f))
                for r in ("default", "fused")}
        ts, out = {"default": [], "fused": []}, {}
        for r in range(args.warmup + args.repeats):
            for route in ("default", "fused"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out[route] = call[route]()
                e1.record()
                torch.cuda.synchronize()
                if r >= args.warmup:
                    ts[route].append(e0.elapsed_time(e1))
        med = {k: statistics.median(v) for k, v in ts.items()}
        cand = int(I.det_candidates(rois, logits, pred, (1024, 1024, 3), sf, True, 0.05)[5])
        # the five kernels of as_det_candidates by themselves: HIP events around back-to-back calls (allocations included)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.repeats):
            I.det_candidates(rois, logits, pred, (1024, 1024, 3), sf, True, 0.05)
        e1.record()
        torch.cuda.synchronize()
        alone.append(f"{n} x {K}: {e0.elapsed_time(e1) / args.repeats:.3f} ms")
        syncs = {k: _count_syncs(call[k]) for k in call}
        launches = {k: _count_launches(call[k]) for k in call}
        (dd, ld), (df, lf) = out["default"], out["fused"]
        same = dd.shape == df.shape and torch.equal(ld, lf) and torch.allclose(dd, df, rtol=1e-5, atol=1e-4)
        notes.append(f"{n} x {K}: {dd.shape[0]} / {df.shape[0]} detections, the same labels and boxes within rtol 1e-5 / atol 1e-4: {same}")
        fmt = lambda v: "not measured" if v is None else str(v)      # noqa: E731
        lines.append(f"| {n} x {K} | {cand} | {med['default']:.3f} ({min(ts['default']):.3f}) | {fmt(launches['default'])} | "
                     f"{syncs['default']} | {med['fused']:.3f} ({min(ts['fused']):.3f}) | {fmt(launches['fused'])} | {syncs['fused']} | "
                     f"{med['default'] / med['fused']:.2f} |")
    lines += ["", "The two routes' detections (default / fused): " + "; ".join(notes) + ".",
              "The fused route's launches are the five of `as_det_candidates`, the two of `as_nms` and torch's gather of the kept rows.",
              f"`det_candidates` alone (five launches, no readback) between HIP events over {args.repeats} back-to-back calls: "
              + "; ".join(alone) + "."]
    return lines


def _host_paste(logits, labels, dets, H, W):
    """the tensor-op route up to the thresholded device tensor (what get_seg_masks does before its copy to the host)"""
    probs = logits.sigmoid()
    sel = probs[torch.arange(probs.shape[0], device=probs.device), labels][:, None]
    return I.paste_masks(sel, dets[:, :4], H, W) >= 0.5          # (AS_POST_HOST=1 is set around this call)


if __name__ == "__main__":
    main()
