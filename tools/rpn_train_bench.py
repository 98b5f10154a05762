"""Times the RPN's training targets and losses at the headline geometry on both routes, in one process on one GPU:

    geometry      1024 x 1024, five levels 256^2 ... 16^2 positions x 3 anchors = 261 888 anchors per image, B = 2
    boxes         G = 3 and G = 20 per image, sized like the RoI head's pseudo boxes (40 ... 500 pixels)
    rpn_assign    inside flags + MaxIoUAssigner (0.7 / 0.3 / 0.3, low-quality matches) alone
    RPNHead.loss  assign, sample (num 256), targets, the two losses, and the backward to the logits and deltas

`device` = csrc/rpn_train.hip, `host` = the tensor-op route on the same device tensors (AS_POST_HOST=1).  Every call is
followed by a device synchronize; the figure is the median of --repeats calls after --warmup, the two routes alternating call
by call.  Also: the HIP-event time of the new kernels over back-to-back calls, and the number of host synchronisations of
one RPNHead.loss call per route (torch.cuda.set_sync_debug_mode).  Prints a markdown table (profiles/rpn_train_bench.md is
this output) and checks that both routes assign every anchor alike.

    python tools/rpn_train_bench.py [--repeats 10] [--warmup 2] [--out profiles/rpn_train_bench.md]
"""
import argparse
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from attentionshift_amd import ops, rpn_train as RT     # noqa: E402
from attentionshift_amd.rpn import RPNHead              # noqa: E402
from post_bench import _route, both_routes              # noqa: E402

STRIDES = [4, 8, 16, 32, 64]
TRAIN_CFG = dict(assigner=dict(type="MaxIoUAssigner", pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True,
                               ignore_iof_thr=-1),
                 sampler=dict(type="RandomSampler", num=256, pos_fraction=0.5, neg_pos_ub=-1, add_gt_as_proposals=False),
                 allowed_border=-1, pos_weight=-1)


def count_syncs(fn):
    """-> host synchronisations of one call of fn"""
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return sum("called a synchronizing" in str(w.message) for w in seen)


def events(fn, repeats):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(repeats):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / repeats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    gen = torch.Generator().manual_seed(4)
    head = RPNHead(256, 256, anchor_generator=dict(type="AnchorGenerator", scales=[8], ratios=[0.5, 1.0, 2.0], strides=STRIDES),
                   loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=True, loss_weight=1.0),
                   loss_bbox=dict(type="L1Loss", loss_weight=1.0), train_cfg=TRAIN_CFG).cuda()
    B, sizes = 2, [(1024 // s, 1024 // s) for s in STRIDES]
    T = sum(3 * h * w for h, w in sizes)
    metas = [dict(img_shape=(1024, 1024, 3), pad_shape=(1024, 1024, 3))] * B
    cls = [(torch.randn(B, 3, h, w, generator=gen) * 2).cuda().requires_grad_() for h, w in sizes]
    reg = [(torch.randn(B, 12, h, w, generator=gen) * 0.2).cuda().requires_grad_() for h, w in sizes]
    base = head.base_anchors
    rows, notes = [], []
    for G in (3, 20):
        xy = torch.rand(B, G, 2, generator=gen) * 600
        gts = [torch.cat((xy[b], xy[b] + 40 + torch.rand(G, 2, generator=gen) * 380), 1).clamp(max=1023).cuda() for b in range(B)]

        def assign(route):
            return RT.rpn_assign(base, sizes, head.anchor_generator.strides, gts, metas, TRAIN_CFG["assigner"], -1)

        def loss(route):
            out = head.loss(cls, reg, gts, metas, generator=torch.Generator().manual_seed(1))
            torch.autograd.grad(sum(out["loss_rpn_cls"]) + sum(out["loss_rpn_bbox"]), cls + reg)
            return out

        a = both_routes(assign, args.repeats, args.warmup)
        ad, ah = a["device"][2], a["host"][2]
        assert ad.device_route and not ah.device_route
        same = torch.equal(ad.assigned, ah.assigned) and torch.equal(ad.max_iou, ah.max_iou) and torch.equal(ad.counts, ah.counts)
        assert same, "the two routes assign differently"
        lo = both_routes(loss, args.repeats, args.warmup)
        ld, lh = lo["device"][2], lo["host"][2]
        diff = max(float((torch.stack(ld[k]) - torch.stack(lh[k])).detach().abs().max()) for k in ld)
        # the kernels alone: HIP events around back-to-back calls (the wrappers' allocations included, no readback)
        smp = RT.rpn_sample(ad, 256, 0.5, -1, torch.Generator().manual_seed(1))
        plan = torch.tensor([[n, 0, m, 0] for n, m in zip(smp.n_pos, smp.n_neg)], dtype=torch.int32).cuda()
        ranks = torch.stack([torch.stack([torch.randperm(max(int(c), 1))[:256].to(torch.int32) if int(c) >= 256 else
                                          torch.arange(256, dtype=torch.int32) % max(int(c), 1) for c in row])
                             for row in ad.counts.cpu()]).cuda()
        t_assign = events(lambda: ops.rpn_assign(base, sizes, head.anchor_generator.strides, ad.gt_cat, ad.gt_offsets, ad.sum_g, G,
                                                 ad.shapes, 0.7, 0.3, 0.3, True, -1), args.repeats)

        def sample_targets():
            inds = ops.rpn_sample(ad.assigned, plan, ranks, ad.workspace, ad.sum_g)
            ops.rpn_targets(base, sizes, head.anchor_generator.strides, ad.gt_cat, ad.gt_offsets, ad.sum_g, ad.assigned, inds)
        t_sample = events(sample_targets, args.repeats)
        _route("device")
        s_dev = count_syncs(lambda: loss("device"))
        _route("host")
        s_host = count_syncs(lambda: loss("host"))
        _route("device")
        counts = ad.counts.tolist()
        for name, r in (("`rpn_assign`", a), ("`RPNHead.loss` forward + backward", lo)):
            rows.append(f"| {name} | {G} | {r['device'][0] * 1e3:.3f} ({r['device'][1] * 1e3:.3f}) | "
                        f"{r['host'][0] * 1e3:.3f} ({r['host'][1] * 1e3:.3f}) | {r['host'][0] / r['device'][0]:.1f} |")
        notes.append(f"G = {G}: (positives, negatives) per image {counts}; `as_rpn_assign` (memset + three launches) {t_assign * 1e3:.3f} ms, "
                     f"`as_rpn_sample` + `as_rpn_targets` (two launches) {t_sample * 1e3:.3f} ms between HIP events over {args.repeats} "
                     f"back-to-back calls; host synchronisations of one `RPNHead.loss` forward + backward: device route {s_dev}, tensor-op "
                     f"route {s_host}; both routes assign all {B * T} anchors alike: {same}; largest loss difference {diff:.2e}.")
    traffic = B * T * 8
    lines = ["# RPN training targets: device kernels against the tensor-op route",
             "",
             f"`python tools/rpn_train_bench.py --repeats {args.repeats} --warmup {args.warmup}` on {torch.cuda.get_device_name(0)}; "
             f"1024 x 1024, levels {' / '.join(f'{h}^2' for h, _ in sizes)} x 3 anchors = {T} anchors per image, B = {B}, the shipped "
             "`train_cfg.rpn` (0.7 / 0.3 / 0.3, low-quality matches, 256 samples, half positive).  Wall time per call including the "
             "device synchronize, median (min) in ms; both routes run on the same device tensors and alternate call by call.",
             "",
             "| stage | boxes per image | device (`csrc/rpn_train.hip`) | tensor-op route (`AS_POST_HOST=1`) | tensor-op / device |",
             "|---|---|---|---|---|"] + rows + [""] + notes + [
             "",
             f"The assignment's per-anchor outputs are {traffic / 1e6:.2f} MB (8 bytes per anchor), written by the first kernel and read and "
             "rewritten by the second; the tensor-op route is new code too, so its column is a comparison, not a bar."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
