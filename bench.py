"""Headline benchmark of the hot path (BASELINE.json: images/sec at 1024^2, ViT-B; kernel rooflines).

    python bench.py --gpus N --steps K --warmup W [--config vitb|vitl|swinb] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N ...

A plain run does what the headline figure needs and no more: set-up, W warm-up steps, K timed steps, the outputs of the
last timed step to DIR when --dump-outputs is given, one JSON line.  Every other leg described below (the extra event-timed
steps, the other RNG mode / precision / configurations, the roll-out check against the dense product, the training step,
the CPU baseline) runs only with --full.

One STEP = one pass of the hot path over one batch.  `--config vitb` (default, the configuration the metric is quoted
on = BASELINE configs[1] per GPU, configs[2] at 8 GPUs): MAE-ViT-Base, 1024x1024, 2 images, 3 point-labelled objects per
image, 7 roll-out layers, 5 mean-shift iterations, bf16:
    VisionTransformerDet.forward (12 blocks: QKV GEMM + flash SDPA + proj, MLP, FPN taps, point head)
  + AttnShiftRoIHead.seed_pseudo_gt (roll-out rows, CAM boxes via CCL, cosine refinement, instance maps,
    mean-shift token clustering, part centres, pseudo masks -> host numpy, exactly as the reference hands
    them to the mask head).
`--config vitl` = BASELINE configs[3] per GPU (MAE-ViT-Large, 1280x1280, 1 image, 7 objects: N = 6501 tokens);
`--config swinb` = BASELINE configs[4] per GPU (Swin-B windowed-attention backbone forward, 1024x1024, 2 images; the
reference's attention shift needs ViT attention maps, so this step is the backbone alone).
Inputs are synthetic and resident in HBM before the timed region.  Because randomly initialised weights give
near-uniform attention, the attention-shift stage consumes the seeded CAM rows / feature blobs of SURVEY 8d
(attentionshift_amd/synthetic.py); the roll-out itself is still computed from the real attention of the pass.
Images shard over GPUs with no data-path collective in this (forward / no-grad) path: weak scaling.

Rank 0 prints ONE JSON line.  `roofline` = the dominant kernel (flash SDPA forward, MFMA-bound) timed with
HIP events on its launch stream inside the timed region; `roofline_affinity` = the mean-shift token-affinity
call (HBM-bound, algorithmic bytes of SURVEY 8d).  With --full: `cpu_baseline` = the CPU oracle port timed on this box's
host cores on a bounded sample (rank 0, N=1 only); `train` = the DDP training step (forward + attention shift + the
RoI head's real losses on seeded proposals + backward + bucketed RCCL gradient all-reduce + AdamW): always at N > 1,
where it is what exercises xGMI, and at N = 1 unless --train-steps 0.  A watchdog prints the headline record without the
training leg if that leg does not finish (so an RCCL problem can never take the scaling number down).

--dump-outputs DIR: after the timed steps rank 0 writes what the LAST timed step handed to its caller as DIR/<name>.npy
(float32; float64 for float64 and 32- / 64-bit integer values): `labels.*` = the dict seed_pseudo_gt returned (boxes, mask points, part centres,
instance maps, pseudo masks, ...), `backbone.*` = the backbone's outputs of the same step (last_feat, FPN maps, point
head).  Arrays above a size cap are a fixed seeded sample of their elements (64 MB in all at most).  Inputs, weights
and the RNG seed are functions of the arguments alone, so two builds run with the same arguments can be compared
array for array.
"""
import argparse
import json
import os
import sys
import threading
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0     # dense bf16 MFMA, MI355X_MICROARCH.md
PEAK_HBM_GBPS = 8000.0

CONFIGS = {
    "vitb": dict(workload="BASELINE configs[1]: MAE-ViT-Base 1024x1024, batch 2/GPU, 3 objects/img, 7 roll-out layers, "
                          "5 shift iters, forward + no-grad attention shift",
                 backbone="vit", img=1024, patch=16, embed_dim=768, depth=12, heads=12, batch=2, objects=3, cam_layer=7,
                 n_shift=5, point_tokens=100, num_classes=20),
    "vitl": dict(workload="BASELINE configs[3] per GPU: MAE-ViT-Large 1280x1280, batch 1/GPU, 7 objects/img (COCO-shaped), "
                          "7 roll-out layers, 5 shift iters, forward + no-grad attention shift",
                 backbone="vit", img=1280, patch=16, embed_dim=1024, depth=24, heads=16, batch=1, objects=7, cam_layer=7,
                 n_shift=5, point_tokens=100, num_classes=80),
    "swinb": dict(workload="BASELINE configs[4] per GPU: Swin-B (embed 128, depths 2/2/18/2, heads 4/8/16/32, window 7) "
                           "1024x1024, batch 2/GPU, backbone forward (windowed attention; no attention-shift stage)",
                  backbone="swin", img=1024, batch=2),
}
CFG = dict(CONFIGS["vitb"])


def head_cfg(full, rng_mode):
    """AttnShiftRoIHead config.  full=False: the attribute-only sub-heads of the pseudo-label path (depth selector =
    median CAM-box area).  full=True: configs/mae/attnshift_voc12aug.py:60-150 with the backbone's width -- the MIL head
    (it then selects the roll-out depth, stdroi:2308-2312), the MAE-decoder box and mask heads and the R-CNN train_cfg."""
    Lc, ncls, D = CFG["cam_layer"], CFG["num_classes"], CFG["embed_dim"]
    cfg = dict(type="AttnShiftRoIHead", num_semantic_points=5, mean_shift_times_local=CFG["n_shift"], rng_mode=rng_mode,
               bbox_head=dict(type="MAEBoxHeadRec", seed_thr=0.2, seed_multiple=0.5, cam_layer=Lc, num_classes=ncls),
               mil_head=dict(type="MAEBoxHeadMIL", num_layers_query=Lc))
    if not full:
        return cfg
    dec = dict(in_channels=D, img_size=224, patch_size=16, embed_dim=256, depth=4, num_heads=8, mlp_ratio=4., num_classes=ncls)
    cfg.update(
        bbox_roi_extractor=dict(type="SingleRoIExtractor", roi_layer=dict(type="RoIAlign", output_size=7, sampling_ratio=0),
                                out_channels=D, featmap_strides=[16]),
        mask_roi_extractor=dict(type="SingleRoIExtractor", roi_layer=dict(type="RoIAlign", output_size=14, sampling_ratio=0),
                                out_channels=D, featmap_strides=[16]),
        mil_head=dict(type="MAEBoxHeadMIL", in_channels=D, embed_dim=256, num_classes=ncls, num_layers_query=Lc,
                      loss_mil_factor=1.0, hidden_dim=1024, roi_size=7),
        bbox_head=dict(type="MAEBoxHeadRec", with_reconstruct=False, seed_score_thr=0.05, seed_thr=0.2, seed_multiple=0.5,
                       cam_layer=Lc, reg_class_agnostic=False, reg_decoded_bbox=True,
                       bbox_coder=dict(type="DeltaXYWHBBoxCoder", target_means=[0.] * 4, target_stds=[.1, .1, .2, .2]),
                       loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0),
                       loss_bbox=dict(type="GIoULoss", loss_weight=10.0), loss_point=dict(type="L1Loss", loss_weight=10.0),
                       loss_point_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0), **dec),
        mask_head=dict(type="MAEMaskHeadPointSup", scale_factor=2, scale_mode="bicubic", **dec),
        train_cfg=dict(assigner=dict(type="MaxIoUAssigner", pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5,
                                     match_low_quality=False),
                       sampler=dict(type="RandomSampler", num=512, pos_fraction=0.25, add_gt_as_proposals=True),
                       point_assigner=dict(type="HungarianPointAssigner", cls_cost=dict(weight=1.0), reg_cost=dict(weight=10.0)),
                       point_pos_weight=1, pos_weight=-1))
    return cfg


def synthetic_proposals(shift, device, n=1000):
    """Seeded stand-in for the RPN's proposals (rpn_proposal max_per_img=1000): jittered copies of the objects' boxes
    (so the IoU assigner finds positives) and uniform boxes, per image [n, 4]."""
    out = []
    for i, s in enumerate(shift):
        g = torch.Generator().manual_seed(7000 + i)
        boxes = s["boxes"]
        k = n // 2 // max(boxes.shape[0], 1)
        jit = boxes.repeat(k, 1) + (torch.rand(boxes.shape[0] * k, 4, generator=g) - 0.5) * 96.0
        xy = torch.rand(n - jit.shape[0], 2, generator=g) * (CFG["img"] - 160)
        rnd = torch.cat((xy, xy + 32 + torch.rand(xy.shape[0], 2, generator=g) * 128), 1)
        b = torch.cat((jit, rnd)).clamp(0, CFG["img"] - 1)
        b[:, 2:] = torch.maximum(b[:, 2:], b[:, :2] + 8)
        out.append(b.to(device))
    return out


def build(device, rng_mode="fast", train=False, ranks=None, mil=False, compute_dtype=torch.bfloat16, check_rollout=True):
    """-> step().  check_rollout=False leaves out the one-time comparison of the first call's roll-out rows with the dense
    product (a plain benchmark run).  The forward steps carry `step.keep`: set it to a dict and every call leaves the
    backbone's outputs and its own return value there (--dump-outputs)."""
    import attentionshift_amd as A
    from attentionshift_amd import synthetic

    torch.manual_seed(0)
    if CFG["backbone"] == "swin":
        bb = A.build_backbone(dict(type="SwinTransformer", embed_dim=128, depths=[2, 2, 18, 2], num_heads=[4, 8, 16, 32],
                                   window_size=7, drop_path_rate=0.3, out_indices=(0, 1, 2, 3)))
        bb.init_weights()
        bb = bb.to(device).eval()
        rank = int(os.environ.get("RANK", "0"))
        img = synthetic.images(CFG["batch"], CFG["img"], CFG["img"], seed=rank).to(device)

        def swin_step():
            res = bb(img)
            if swin_step.keep is not None:
                swin_step.keep.update(backbone=res, labels=None)
            return res

        swin_step.head = None
        swin_step.keep = None
        return swin_step

    bb = A.build_backbone(dict(type="VisionTransformerDet", img_size=CFG["img"], patch_size=CFG["patch"],
                               embed_dim=CFG["embed_dim"], depth=CFG["depth"], num_heads=CFG["heads"], mlp_ratio=4.,
                               qkv_bias=True, drop_path_rate=0.05, out_indices=(3, 5, 7, 11) if CFG["depth"] == 12 else (5, 11, 17, 23),
                               learnable_pos_embed=True, use_checkpoint=True, last_feat=True,
                               point_tokens_num=CFG["point_tokens"], num_classes=CFG["num_classes"], return_attention=True,
                               compute_dtype=compute_dtype, defer_fpn=not train and os.environ.get("AS_DEFER_FPN", "0") == "1",
                               point_head_stream=not train and os.environ.get("AS_POINT_HEAD_STREAM", "0") == "1"))
    bb = bb.to(device)
    bb = bb.train() if train else bb.eval()

    hp = wp = CFG["img"] // CFG["patch"]
    G, Lc, T, B = CFG["objects"], CFG["cam_layer"], CFG["point_tokens"], CFG["batch"]
    rank = int(os.environ.get("RANK", "0"))                # every rank works on its own images (weak scaling)
    shift = [synthetic.shift_inputs(1234 + rank * B + b, hp, wp, CFG["embed_dim"], G, Lc) for b in range(B)]
    cams = torch.stack([s["cams"].flatten(2) for s in shift]).to(device)          # [B, Lc, G, Np]
    # vit_feat reaches seed_pseudo_gt the way the reference's caller builds it (two_stage_point_align.py:77): a
    # permuted VIEW [B, C, hp, wp] of the token-major last_feat [B, 1 + Np, C] with the cls row dropped
    last = torch.zeros(B, 1 + hp * wp, CFG["embed_dim"])
    last[:, 1:] = torch.stack([s["vit_feat"].flatten(1).t() for s in shift])
    vit_feat = last.to(device).permute(0, 2, 1)[..., 1:].unflatten(-1, (hp, wp))
    gt_points = [s["points"].to(device) for s in shift]
    gt_labels = [(s["labels"] % CFG["num_classes"]).to(device) for s in shift]

    class BenchHead(A.AttnShiftRoIHead):
        # set by the FIRST call (a warm-up step): the real rows vs the dense route; False = the check is not wanted
        rollout_check = None if check_rollout else False

        def rollout_cams(self, attns, num_proposals, pos_inds=None):
            rows = super().rollout_cams(attns, num_proposals, pos_inds)         # real roll-out of this pass
            if self.rollout_check is None:
                # the rows are replaced by seeded CAMs below (random-init weights give near-uniform attention), so the
                # values the roll-out kernels produced are checked HERE, once, against the dense head-mean product
                # (as_attn_mean_rows + fp32 torch matmuls); bf16 operands: 3e-2 of the range, as the parity tests
                from attentionshift_amd import ops as _ops
                sel = None
                if getattr(self, "_rows_matched_only", False):
                    sel = torch.stack([p for p in pos_inds]).to(rows.device).long()
                ref = _ops.rollout_rows_dense(attns[-self.bbox_head.cam_layer:], num_proposals, rows=sel)
                scale = float(ref.abs().max()) + 1e-30
                err = (ref - rows).abs()
                self.rollout_check = dict(max_rel=float(err.max()) / scale, mean_rel=float(err.mean()) / scale,
                                                rows=list(rows.shape), vs="as_attn_mean_rows dense product (fp32 matmul)")
                if not (self.rollout_check["max_rel"] < 3e-2):
                    raise RuntimeError(f"roll-out rows differ from the dense product: {self.rollout_check}")
                del ref, err
            rows[:, :, :G, 1:-num_proposals] = cams                              # seeded, non-degenerate CAMs
            return rows

    cfg = head_cfg(train or mil, rng_mode)
    cfg.pop("type")
    head = BenchHead(**cfg).to(device)
    head.ranks = ranks
    img = synthetic.images(B, CFG["img"], CFG["img"], seed=rank).to(device)
    metas = [dict(img_shape=(CFG["img"], CFG["img"], 3)) for _ in range(B)]
    pos_inds = [torch.arange(G, device=device) for _ in range(B)]
    seed_kw = dict(return_mask=True, pos_mask_thr=0.35, neg_mask_thr=0.8, num_mask_point_gt=10, corr_size=21, obj_tau=0.9,
                   pos_inds=pos_inds, matched_gt=pos_inds)

    def pseudo_labels(out):
        return head.seed_pseudo_gt(out["feature"], metas, None, None, None, vit_feat=vit_feat, img=img,
                                   point_cls=out["outputs_class"], point_reg=out["outputs_coord"], attns=out["attns"],
                                   gt_points=gt_points, gt_points_labels=gt_labels, point_ready=out.get("point_head_ready"),
                                   roi_feature_map=out["feature"][2].float() if mil else None, **seed_kw)

    if not train:
        def step():
            out = bb(img)
            res = pseudo_labels(out)
            if hasattr(out["feature"], "result"):
                out["feature"].result()                # the step ends with the FPN maps valid on the caller's stream
            if "point_head_ready" in out:              # ... and the point head's outputs (queued on its own stream)
                torch.cuda.current_stream().wait_event(out["point_head_ready"])
            if step.keep is not None:
                step.keep.update(backbone=out, labels=res)
            return res

        step.head = head
        step.keep = None
        return step

    # DDP training step (BASELINE configs[2] shape per GPU; mmdet/apis/train.py:95-100 + two_stage_point_align.py:75-157
    # with precomputed proposals): backbone forward under autograd (HIP attention fwd), the no-grad attention shift on its
    # outputs, the RoI head's REAL losses against the pseudo labels (MIL, point-token, box, point-supervised mask) on the
    # stride-16 feature map, backward (HIP attention bwd), bucketed RCCL gradient all-reduce overlapped with backward,
    # one fused all-reduce of the logged scalars, AdamW.  (The RPN / FPN neck that would produce the proposals is not part
    # of this build; the proposals are seeded jitters of the objects' boxes.)
    from attentionshift_amd.dist import GradAllReducer, convert_sync_batchnorm, parse_losses
    if ranks is not None and ranks.dist is not None:
        convert_sync_batchnorm(bb, ranks)              # as mmdet/apis/train.py:95 does before wrapping the model in DDP
    head.train()
    params = [p for p in list(bb.parameters()) + list(head.parameters()) if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=1e-4, weight_decay=0.05, fused=True)
    # rank 0's parameters AND buffers are broadcast at construction (mmdet/apis/train.py:96-100); fp32 wire by default
    comm = getattr(torch, os.environ.get("AS_COMM_DTYPE", "float32"))
    reducer = GradAllReducer(params, ranks, comm_dtype=comm, buffers=list(bb.buffers()) + list(head.buffers()))
    proposals = synthetic_proposals(shift, device)
    gen = torch.Generator().manual_seed(99 + rank)

    train_kw = {k: v for k, v in seed_kw.items() if k != "return_mask"}       # train_losses always asks for the masks

    def micro_step(scale):
        out = bb(img)
        fmap = out["feature"][2].float()               # the stride-16 map the RoI extractors read (roi_skip_fpn=True)
        # the heads' Linear layers in bf16 (the reference trains under apex O1: fp16 GEMMs, fp32 norms / losses)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            losses, labels = head.train_losses(fmap, metas, proposals, vit_feat, out["attns"], out["outputs_class"].float(),
                                               out["outputs_coord"].float(), gt_points, gt_labels, generator=gen, **train_kw)
        loss, log_vars = parse_losses(losses, ranks, lazy=True)       # read back after the step has been queued
        (loss * scale if scale != 1.0 else loss).backward()
        return log_vars

    finish_events = []                                   # (start, end) CUDA events around reducer.finish()

    def train_step(update_interval=1, grad_clip=None):
        """One OPTIMIZER step = `update_interval` micro-batches (mmdet/utils/optimizer.py:23-38 DistOptimizerHook: the loss
        of each is divided by update_interval, gradients accumulate, clip / step / zero_grad on the last one; the
        reference runs update_interval=2, run_train.py:13).  Micro-steps before the last run under no_sync(): one
        gradient all-reduce per optimizer step."""
        for i in range(update_interval - 1):
            with reducer.no_sync():
                micro_step(1.0 / update_interval)
        log_vars = micro_step(1.0 / update_interval)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        reducer.finish()
        e1.record()
        finish_events.append((e0, e1))
        if grad_clip is not None:
            torch.nn.utils.clip_grad_norm_(params, **grad_clip)
        opt.step()
        opt.zero_grad(set_to_none=True)                    # (torch's default, what the reference's optimizer hook calls)
        return log_vars.resolve()                          # the logged scalars: the step's last host sync

    train_step.head = head
    train_step.reducer = reducer
    train_step.finish_events = finish_events
    return train_step


def _static_traffic(names, key):
    """HBM bytes per call from the PMC passes kept under profiles/ (FETCH_SIZE x 2 + WRITE_SIZE, separate rocprofv3 --pmc
    runs, tools/pmc_call_traffic.sh): a pointer to the NEWEST committed measurement of the same shape and kernel -- PMC
    collection needs its own rocprofv3 passes, so it cannot happen inside this run; the file and its round are named."""
    for name in names:
        path = os.path.join(ROOT, "profiles", name)
        try:
            with open(path) as f:
                d = json.load(f)
            return {"bytes": float(d[key]), "source": f"profiles/{name} (separate rocprofv3 --pmc passes of the same call; "
                                                      f"{d.get('note', 'committed with the round named in the file')})"}
        except (OSError, KeyError, ValueError):
            continue
    return None


def cpu_baseline(only_threads=None):
    """The CPU oracle (a port of the reference's PyTorch path) on this box's host cores, bounded sample per BASELINE.md
    section 3: ONE image; 1 of the 12 ViT-B blocks at N=4197 incl. the dense head-mean attention the reference keeps
    (extrapolated x12), the 7-layer row roll-out and the full attention-shift chain (G=3, S=5); 1 warm-up + 3 timed runs,
    median."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import attnshift_oracle as O
    from attentionshift_amd import synthetic

    # many-core hosts thrash on the small ops of this path: cap the pool and report both numbers
    host_cores = os.cpu_count() or 1
    c = CONFIGS["vitb"]
    D, h, T = c["embed_dim"], c["heads"], c["point_tokens"]
    hp = wp = c["img"] // c["patch"]
    N = 1 + hp * wp + T
    p = "blocks.0."
    shapes = {p + "norm1.weight": (D,), p + "norm1.bias": (D,), p + "attn.qkv.weight": (3 * D, D),
              p + "attn.qkv.bias": (3 * D,), p + "attn.proj.weight": (D, D), p + "attn.proj.bias": (D,),
              p + "norm2.weight": (D,), p + "norm2.bias": (D,), p + "mlp.fc1.weight": (4 * D, D),
              p + "mlp.fc1.bias": (4 * D,), p + "mlp.fc2.weight": (D, 4 * D), p + "mlp.fc2.bias": (D,)}
    sd = synthetic.det_state_dict(shapes)
    inp = synthetic.shift_inputs(1234, hp, wp, D, c["objects"], c["cam_layer"])
    x0 = torch.randn(1, N, D, generator=torch.Generator().manual_seed(0))

    def one_run():
        with torch.no_grad():
            t0 = time.time()
            _x, pr = O.block(x0, sd, p, h)
            attn = pr.mean(1)
            t_block = time.time() - t0
            t0 = time.time()
            O.rollout_rows([attn] * c["cam_layer"], T)
            t_roll = time.time() - t0
            torch.manual_seed(1)
            t0 = time.time()
            boxes, cams_up = O.cam_boxes_from_rollout(inp["cams"], inp["points"], 0.2, 0.5)
            best = torch.zeros(c["objects"], dtype=torch.long)
            rois = boxes[torch.arange(c["objects"]), best]
            attn_sel = cams_up[best, torch.arange(c["objects"])]
            fg, bg = O.sample_refine_inputs(attn_sel, inp["points"])
            m_fg, m_bg, _, _ = O.cosine_refined_maps(attn_sel, inp["vit_feat"], rois, fg, bg, 2, 0.9)
            O.mask_sample_points(m_fg[-1], m_bg[-1], rois, 0.35, 0.8, 10, 21)
            O.semantic_centers(m_fg[-1], m_bg[-1], rois, inp["vit_feat"], 0.35, c["n_shift"], inp["labels"], num_semantic_points=5)
            O.pseudo_masks(m_fg[-1], 0.35)
            t_shift = time.time() - t0
        return t_block, t_roll, t_shift

    # BASELINE.md section 3 asks for torch.set_num_threads(os.cpu_count()).  On a 256-thread host these mostly small ops
    # thrash with that many threads (measured: 160 s per image against 6.7 s with 32), so the sample is timed with a
    # 32-thread pool in this process and with every host thread in a child process under a 30 s limit; the faster
    # setting is the reported baseline, both outcomes are recorded.
    def sample(threads, max_runs=3):
        torch.set_num_threads(threads)
        t0 = time.time()
        one_run()                                       # warm-up
        n_runs = max_runs if time.time() - t0 < 6.0 else 1
        runs = sorted((one_run() for _ in range(n_runs)), key=lambda r: r[0] * c["depth"] + r[1] + r[2])
        t_block, t_roll, t_shift = runs[len(runs) // 2]     # median
        return (t_block * c["depth"] + t_roll + t_shift, torch.get_num_threads(), t_block, t_roll, t_shift, n_runs)

    if only_threads is not None:                        # child process of the all-threads leg (see below)
        r = sample(only_threads, max_runs=1)
        print(json.dumps({"cpu_sample": list(r)}), flush=True)
        return None
    rates = {}
    best = sample(min(host_cores, 32))
    rates[str(best[1])] = round(1.0 / best[0], 4)
    import subprocess
    # more threads, each count in a child process with a hard time limit (the parent cannot interrupt a torch op): 64 when
    # the host has them (one more data point between the 32-thread pool and the whole machine) and every host thread
    for threads, limit in [(t, l) for t, l in ((64, 20.0), (host_cores, 30.0)) if host_cores > 32 and t <= host_cores and t > 32]:
        try:
            cp = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-sample", str(threads)], capture_output=True,
                                text=True, timeout=limit, env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))
            line = [ln for ln in cp.stdout.splitlines() if ln.startswith('{"cpu_sample"')]
            full = tuple(json.loads(line[-1])["cpu_sample"]) if line else None
        except subprocess.TimeoutExpired:
            full = None
        if full is not None:
            rates[str(int(full[1]))] = round(1.0 / full[0], 4)
            if full[0] < best[0]:
                best = full
        else:
            rates[f"{threads}: the sample did not finish within {limit:.0f}s"] = None
    per_image, cores, t_block, t_roll, t_shift, n_runs = best

    # The reference's LITERAL arithmetic for the two stages the port restates more cheaply (ONE run each, same thread pool):
    # the six dense N x N x N roll-out products of stdroi:1257-1272 (`rollout_full`; the port slices the 100 point rows
    # first) and every cosine of the chain as the broadcast F.cosine_similarity of stdroi:832 (`faithful=True`; the port
    # uses a normalised matmul).  Reported beside the port, not instead of it.
    literal = None
    if os.environ.get("AS_BENCH_LITERAL", "1") == "1":
        try:
            torch.set_num_threads(int(cores))
            with torch.no_grad():
                attn = torch.softmax(torch.randn(1, N, N, generator=torch.Generator().manual_seed(2)), -1)
                t0 = time.time()
                O.rollout_full([attn] * c["cam_layer"])
                t_roll_lit = time.time() - t0
                del attn
                torch.manual_seed(1)
                boxes, cams_up = O.cam_boxes_from_rollout(inp["cams"], inp["points"], 0.2, 0.5)
                bestl = torch.zeros(c["objects"], dtype=torch.long)
                rois = boxes[torch.arange(c["objects"]), bestl]
                attn_sel = cams_up[bestl, torch.arange(c["objects"])]
                fg, bg = O.sample_refine_inputs(attn_sel, inp["points"])
                m_fg, m_bg, _, _ = O.cosine_refined_maps(attn_sel, inp["vit_feat"], rois, fg, bg, 2, 0.9)
                t0 = time.time()
                O.semantic_centers(m_fg[-1], m_bg[-1], rois, inp["vit_feat"], 0.35, c["n_shift"], inp["labels"],
                                   num_semantic_points=5)
                t_sem_port = time.time() - t0
                t0 = time.time()
                O.semantic_centers(m_fg[-1], m_bg[-1], rois, inp["vit_feat"], 0.35, c["n_shift"], inp["labels"],
                                   num_semantic_points=5, faithful=True)
                t_shift_lit = time.time() - t0
            lit_image = t_block * c["depth"] + t_roll_lit + (t_shift - min(t_sem_port, t_shift) + t_shift_lit)
            literal = dict(images_per_sec=round(1.0 / lit_image, 4), threads=int(cores),
                           rollout_full_s=round(t_roll_lit, 2), rollout_rows_port_s=round(t_roll, 2),
                           mean_shift_faithful_s=round(t_shift_lit, 2), mean_shift_port_s=round(t_sem_port, 2),
                           what="1 run: the dense 7-layer N^3 roll-out (stdroi:1257-1272) in place of the row-sliced one, and the "
                                "mean-shift / part-centre stage with the reference's broadcast cosine (stdroi:832) in place of the "
                                "port's normalised matmul; everything else as the port")
        except Exception as e:                              # noqa: BLE001 -- a baseline detail must not lose the record
            literal = {"error": f"{type(e).__name__}: {e}"[:200]}
    return dict(value=round(1.0 / per_image, 4), unit="images/sec", cores=cores, host_cores=host_cores, kind="port",
                reference_literal=literal, images_per_sec_by_threads=rates,
                sample=(f"1 image, 1 warm-up + {n_runs} run(s) (median): 1/12 ViT-B blocks at N={N} with dense head-mean attention "
                        f"({t_block:.2f}s, x12), 7-layer row roll-out ({t_roll:.2f}s), full attention-shift chain G=3 S=5 "
                        f"({t_shift:.2f}s); timed with {' and '.join(rates)} torch threads on {host_cores} host cores, faster one reported"))


DUMP_BYTES = 60 * 10 ** 6              # --dump-outputs: the arrays of one dump (64 MB with room for the file headers)
DUMP_ARRAY_ELEMS = 1 << 19            # ... and one array above this many elements is written as a sample of that size
BACKBONE_OUTPUTS = ("last_feat", "feature", "org_feats", "point_tokens", "outputs_class", "outputs_coord")


def output_leaves(obj, prefix):
    """Flatten what a step returned (dicts / lists / tuples of tensors, numpy arrays and numbers) into [(name, array-like)]
    with dotted names; a list of plain numbers is one array.  Anything else (None, strings, opaque state) is left out."""
    import numpy as np
    if isinstance(obj, (torch.Tensor, np.ndarray)):
        return [(prefix, obj)]
    if isinstance(obj, (bool, int, float, np.number)):
        return [(prefix, np.asarray(obj))]
    if isinstance(obj, dict):
        return [leaf for k in sorted(obj, key=str) for leaf in output_leaves(obj[k], f"{prefix}.{k}")]
    if isinstance(obj, (list, tuple)):
        if obj and all(isinstance(v, (bool, int, float, np.number)) for v in obj):
            return [(prefix, np.asarray(obj))]
        return [leaf for i, v in enumerate(obj) for leaf in output_leaves(v, f"{prefix}.{i}")]
    return []


def dump_outputs(keep, path):
    """Write the outputs of one step (step.keep) as path/<name>.npy; see the module docstring.  -> {name: shape}."""
    import numpy as np
    bb_out = keep.get("backbone")
    if isinstance(bb_out, dict):
        bb_out = {k: (v.result() if hasattr(v, "result") else v) for k, v in bb_out.items() if k in BACKBONE_OUTPUTS}
    leaves = output_leaves(keep.get("labels"), "labels") + output_leaves(bb_out, "backbone")
    sizes = [int(np.prod(v.shape)) for _, v in leaves]
    cap = DUMP_ARRAY_ELEMS
    while sum(min(n, cap) for n in sizes) * 8 > DUMP_BYTES:       # (many large arrays: smaller samples of each)
        cap = cap * 3 // 4
    os.makedirs(path, exist_ok=True)
    if torch.cuda.is_initialized():
        torch.cuda.synchronize()
    written, total = {}, 0
    for name, v in leaves:
        t = v.detach() if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))
        shape = list(t.shape)
        if t.numel() > cap:              # a fixed sample: the same (sorted, seeded) flat indices for every array of this size
            idx = np.sort(np.random.default_rng(0).integers(0, t.numel(), size=cap))
            t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
        wide = t.dtype in (torch.float64, torch.int64, torch.int32)          # (integers stay exact in float64)
        arr = t.to(torch.float64 if wide else torch.float32).cpu().numpy()
        np.save(os.path.join(path, name + ".npy"), arr)
        written[name] = shape
        total += arr.nbytes
    assert total <= DUMP_BYTES, total
    return written


def timed(step, ranks, steps, per_rank=None):
    """K steps between barrier + synchronize on both sides; MAX over ranks.  per_rank (a dict) additionally receives each
    rank's own time up to its synchronize (before the closing barrier): the spread that the max hides."""
    ranks.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    own = time.perf_counter() - t0
    ranks.barrier()
    total = ranks.max_over_ranks(time.perf_counter() - t0)
    if per_rank is not None:
        per_rank["min_ms_per_step"] = round(-ranks.max_over_ranks(-own) / steps * 1e3, 3)
        per_rank["max_ms_per_step"] = round(ranks.max_over_ranks(own) / steps * 1e3, 3)
    return total


def launch_plan(gpus, env, argv, n_devices, script=None):
    """What `--gpus N` means for this process (the flag used to be decorative).  Returns
        ("run", None)        this process is a rank (or the single process of N = 1): go on
        ("spawn", cmd)       N > 1 and no launcher in the environment: re-execute under torch.distributed.run, one rank
                             per GPU on 127.0.0.1 (what the driver does itself for N > 1)
        ("error", message)   the request cannot be honoured: fail loudly instead of measuring one rank
    Pure function of its arguments (tests/test_host_logic.py covers it without a GPU)."""
    world = int(env.get("WORLD_SIZE", "0") or 0)
    if gpus < 1:
        return "error", f"--gpus {gpus}: need at least one GPU"
    if world == 0:                                          # no launcher
        if gpus == 1:
            return "run", None
        if n_devices < gpus and not env.get("AS_BENCH_SHARE_GPUS"):
            return "error", (f"--gpus {gpus} but this node exposes {n_devices} GPU(s); one rank per GPU is the contract "
                             f"(AS_BENCH_SHARE_GPUS=1 lets ranks share devices for a plumbing check)")
        port = env.get("MASTER_PORT") or str(29500 + os.getpid() % 2000)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}", "--master-addr",
               "127.0.0.1", "--master-port", port, script or os.path.abspath(__file__)] + list(argv)
        return "spawn", cmd
    if world != gpus:
        return "error", f"--gpus {gpus} but the launcher started WORLD_SIZE={world} ranks: the record would misreport n_gpus"
    if n_devices < min(gpus, int(env.get("LOCAL_WORLD_SIZE", gpus) or gpus)) and not env.get("AS_BENCH_SHARE_GPUS"):
        return "error", f"{world} ranks on a node with {n_devices} GPU(s) (set AS_BENCH_SHARE_GPUS=1 for a plumbing check)"
    return "run", None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", choices=sorted(CONFIGS), default="vitb")
    ap.add_argument("--full", action="store_true",
                    help="also run every leg beside the headline: extra event-timed steps, the other RNG mode, the fp32 path, the "
                         "MIL selector, the other configurations, the roll-out check, the training step, the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step as DIR/<name>.npy (rank 0)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-sample", type=int, default=0, help=argparse.SUPPRESS)     # child mode of cpu_baseline()
    ap.add_argument("--train-steps", type=int, default=5, help="steps of the DDP training-step leg (0 = skip)")
    ap.add_argument("--train-timeout", type=float, default=240.0, help="seconds before the watchdog gives up on the training leg")
    ap.add_argument("--train-accum", type=int, default=2, help="update_interval of the accumulation variant of the training leg (1 = skip)")
    ap.add_argument("--other-configs", default="vitl,swinb", help="short forward legs of the other BASELINE configs ('' = none)")
    a = ap.parse_args()
    if a.cpu_sample > 0:
        cpu_baseline(only_threads=a.cpu_sample)
        return
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    what, arg = launch_plan(a.gpus, os.environ, sys.argv[1:], torch.cuda.device_count())
    if what == "error":
        print(f"bench.py: {arg}", file=sys.stderr, flush=True)
        sys.exit(2)
    if what == "spawn":                                     # python bench.py --gpus N without a launcher: become the launcher
        import subprocess
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        sys.exit(subprocess.call(arg, env=env))
    CFG.clear()
    CFG.update(CONFIGS[a.config])

    # stdout carries the ONE JSON line and nothing else: gloo and RCCL print banners to the C-level stdout (RCCL's version
    # block is flushed at process exit, i.e. AFTER the record), so file descriptor 1 is pointed at stderr for the whole
    # run and the record is written to the saved descriptor
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    local = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("AS_BENCH_SHARE_GPUS"):            # test hook: more ranks than GPUs (plumbing check on a 1-GPU box)
        local %= max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    from attentionshift_amd.dist import Ranks
    ranks = Ranks(device=device)       # gloo for host scalars + "nccl" (= RCCL on ROCm) for device tensors (dist.Ranks)
    world, rank = ranks.world, ranks.rank
    if world != a.gpus:                                     # (launch_plan checked the environment; this checks the group itself)
        print(f"bench.py: process group has {world} ranks but --gpus {a.gpus}", file=sys.stderr, flush=True)
        sys.exit(2)

    from attentionshift_amd import ops
    # the host side of this path is a single Python thread; a 256-thread intra-op pool only adds spin-wait noise
    torch.set_num_threads(int(os.environ.get("AS_HOST_THREADS", "8")))
    # Sampling draws: "fast" = draws on the device with the reference's distributions (one readback per image);
    # "reference" = the literal torch.randperm / randint stream of the reference on the host.  The headline number uses
    # AS_RNG_MODE (default fast); the reference-stream rate is measured right after and reported next to it.
    rng_mode = os.environ.get("AS_RNG_MODE", "fast")
    vit = CFG["backbone"] == "vit"
    step = build(device, rng_mode, check_rollout=a.full)
    if a.dump_outputs and rank == 0:
        step.keep = {}
    with torch.no_grad():
        for _ in range(a.warmup):
            step()
        if vit and os.environ.get("AS_BENCH_EVENTS", "1") == "1":
            ops.enable_timing(["sdpa_fwd", "cosine_shift"])
        elif not vit and os.environ.get("AS_BENCH_EVENTS", "1") == "1":
            ops.enable_timing(["window_attn_fwd"])
        elapsed = timed(step, ranks, a.steps)
    timing = ops.collect_timing()
    ops.disable_timing()
    dumped = None
    if step.keep is not None:
        dumped = dump_outputs(step.keep, a.dump_outputs)
        step.keep = None
    block_timing = {}
    if a.full and vit and os.environ.get("AS_BENCH_EVENTS", "1") == "1":
        # the attention BLOCK (A1 + A2 = QKV projection + SDPA + output projection) against the MFMA peak.  Its
        # three launches are timed in a few extra steps AFTER the headline's timed region (six event records per layer would
        # otherwise sit inside it)
        with torch.no_grad():
            ops.enable_timing(["qkv_gemm", "sdpa_fwd", "proj_gemm"])
            for _ in range(5):
                step()
            torch.cuda.synchronize()
        block_timing = ops.collect_timing()
        ops.disable_timing()
        # the affinity call ALONE on the device: in the timed region it shares the chip with the per-image mask-point kernels
        # (AttnShiftRoIHead.overlap_mask_work), which is faster for the step and slower for the call
        if getattr(step, "head", None) is not None and hasattr(step.head, "overlap_mask_work"):
            with torch.no_grad():
                step.head.overlap_mask_work = False
                step()
                ops.enable_timing(["cosine_shift"])
                for _ in range(5):
                    step()
                torch.cuda.synchronize()
                step.head.overlap_mask_work = True
            block_timing["cosine_shift_alone"] = ops.collect_timing().get("cosine_shift")
            ops.disable_timing()
    B = CFG["batch"]
    rec = {
        "metric": "images/sec (1024^2, ViT-B) hot path: backbone attention fwd + attention-shift pseudo-labels",
        "value": round(world * B * a.steps / elapsed, 3), "unit": "images/sec", "n_gpus": world, "steps": a.steps,
        "warmup": a.warmup, "ms_per_step": round(elapsed / a.steps * 1e3, 3), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
        "precision": "bf16 operands / fp32 accumulation (the reference runs fp16 under apex O1). Parity bar of THIS path: 3e-2 of "
                     "the output range vs the fp32 oracle (tests/test_gpu_path.py); north_star's 1e-3 is met by the fp32 path "
                     "(compute_dtype=float32, tests/test_gpu_path.py::test_backbone_*), which is not what is timed; integer / "
                     "index outputs are bit-exact in both",
        "config": {"workload": CFG["workload"], "name": a.config, "global_batch": world * B,
                   "parallelism": f"dp{world} (image sharding, no data-path collective)"},
        "full": a.full,
    }
    if dumped is not None:
        rec["dumped_outputs"] = {"dir": a.dump_outputs, "arrays": len(dumped)}
    if not vit and "window_attn_fwd" in timing:
        # Swin (config 5): the fused window attention is HBM-bound -- its algorithmic traffic is one read of the qkv grid
        # and one write of the output (49 x 49 x 32 per window-head of MFMA work is ~1 % of the matrix peak)
        n_wa, ms_wa = timing["window_attn_fwd"]
        _, bytes_wa = timing.get("window_attn_fwd:bytes", (0, float("nan")))
        gbps_wa = bytes_wa / (ms_wa * 1e-3) / 1e9
        rec["roofline"] = {
            "kernel": "as_window_attn_fwd (bf16, window_attn_mfma_kernel): mean over the 24 launches of a pass "
                      "(stage 1: 134 MB per launch ... stage 4: 8 MB)",
            "bound": "hbm", "achieved": round(gbps_wa, 1), "peak": PEAK_HBM_GBPS, "unit": "GB/s",
            "frac": round(gbps_wa / PEAK_HBM_GBPS, 4), "traffic": None, "launches_timed": n_wa,
            "ms_per_launch": round(ms_wa, 4), "algorithmic_bytes_per_launch": bytes_wa}
    if vit:
        rec["rng_mode"] = rng_mode
        # the real roll-out rows of the first warm-up pass against the dense head-mean product (BenchHead.rollout_cams)
        if a.full:
            rec["rollout_check"] = getattr(step.head, "rollout_check", None)
        other = "reference" if rng_mode == "fast" else "fast"
        if a.full and os.environ.get("AS_BENCH_OTHER_RNG", "1") == "1":      # (0: profiling runs that want the headline leg alone)
            step.head.rng_mode = other
            with torch.no_grad():
                step()
                rec[f"images_per_sec_{other}_rng"] = round(world * B * a.steps / timed(step, ranks, a.steps), 3)
            step.head.rng_mode = rng_mode
        N, h = 1 + (CFG["img"] // CFG["patch"]) ** 2 + CFG["point_tokens"], CFG["heads"]
        n_sdpa, ms_sdpa = timing.get("sdpa_fwd", (0, float("nan")))
        flops_sdpa = 4.0 * B * h * N * N * 64                      # QK^T + PV per launch (one layer, one batch)
        ach = flops_sdpa / (ms_sdpa * 1e-3) / 1e12
        n_cs, ms_cs = timing.get("cosine_shift", (0, float("nan")))
        Np, C, S, G, P = (CFG["img"] // CFG["patch"]) ** 2, CFG["embed_dim"], CFG["n_shift"], CFG["objects"], 20
        imgs_per_call = max(1, round(B * a.steps / max(n_cs, 1)))         # the head batches a step's images into one call
        bytes_cs = imgs_per_call * ((2 * S + 1) * Np * C * 4 + G * P * Np * 4)   # SURVEY 8d, per call
        gbps = bytes_cs / (ms_cs * 1e-3) / 1e9
        headline = a.config == "vitb"
        rec["roofline"] = {
            "kernel": "as_sdpa_fwd (bf16): sdpa_fwd_pipe_kernel (software-pipelined units of 32x32 scores, reference-free "
                      "first pass); 512-row workgroups of 8 waves / 256-row of 4 (64 queries per wave) or 128-row workgroups + "
                      "key-split last q-tile, whichever csrc/sdpa.hip sdpa_pick() prices cheaper for the shape; one timed "
                      "'launch' = the whole call",
            "bound": "mfma", "achieved": round(ach, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
            "frac": round(ach / PEAK_BF16_TFLOPS, 4),
            "traffic": _static_traffic(("r06_sdpa_traffic.json", "r05_sdpa_traffic.json", "r04_sdpa_traffic.json", "r03_sdpa_traffic.json"), "per_as_sdpa_fwd_call_bytes") if headline else None,
            "launches_timed": n_sdpa, "ms_per_launch": round(ms_sdpa, 4), "flops_per_launch": flops_sdpa}
        if all(k in block_timing for k in ("qkv_gemm", "sdpa_fwd", "proj_gemm")):
            D_ = CFG["embed_dim"]
            ms_q, ms_s, ms_p = (block_timing[k][1] for k in ("qkv_gemm", "sdpa_fwd", "proj_gemm"))
            fl_q, fl_p = 2.0 * B * N * D_ * 3 * D_, 2.0 * B * N * D_ * D_
            blk = (fl_q + flops_sdpa + fl_p) / ((ms_q + ms_s + ms_p) * 1e-3) / 1e12
            rec["roofline_attention_block"] = {
                "what": "A1 + A2 of SURVEY 8d(ii): as_qkv_fwd + as_sdpa_fwd + output projection of one layer, one batch "
                        f"({(fl_q + flops_sdpa + fl_p) * CFG['depth'] / B / 1e9:.1f} GFLOP per image forward over the "
                        f"{CFG['depth']} layers); HIP events around the three launches in 5 steps after the timed region",
                "bound": "mfma", "achieved": round(blk, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                "frac": round(blk / PEAK_BF16_TFLOPS, 4), "launches_timed": block_timing["sdpa_fwd"][0],
                "ms_per_layer": {"qkv": round(ms_q, 4), "sdpa": round(ms_s, 4), "proj": round(ms_p, 4),
                                 "sum": round(ms_q + ms_s + ms_p, 4)},
                "frac_by_kernel": {"qkv": round(fl_q / (ms_q * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4),
                                   "sdpa": round(flops_sdpa / (ms_s * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4),
                                   "proj": round(fl_p / (ms_p * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4)},
                "flops_per_layer": fl_q + flops_sdpa + fl_p}
        # the step as a whole against the MFMA peak: the backbone's matrix FLOPs (QKV / proj / MLP GEMMs + QK^T and PV of the
        # attention; the roll-out's recomputed QK^T tiles counted too) over the measured step time
        D, L, Ntok = CFG["embed_dim"], CFG["depth"], N
        gemm_fl = L * 2.0 * B * Ntok * (3 * D * D + D * D + 8 * D * D)
        attn_fl = L * flops_sdpa
        roll_fl = (CFG["cam_layer"] - 1) * 2.0 * B * h * Ntok * Ntok * 64
        step_s = elapsed / a.steps
        rec["step_mfma"] = {"gemm_tflop": round(gemm_fl / 1e12, 4), "attention_tflop": round(attn_fl / 1e12, 4),
                            "rollout_qk_tflop": round(roll_fl / 1e12, 4),
                            "achieved_tflops": round((gemm_fl + attn_fl + roll_fl) / step_s / 1e12, 1),
                            "frac_of_peak": round((gemm_fl + attn_fl + roll_fl) / step_s / 1e12 / PEAK_BF16_TFLOPS, 4),
                            "attention_only_frac": round(attn_fl / step_s / 1e12 / PEAK_BF16_TFLOPS, 4),
                            "what": "matrix FLOPs of one step (12 blocks: QKV + proj + MLP GEMMs, QK^T + PV; 6 roll-out steps' "
                                    "recomputed QK^T) / ms_per_step / 2.5 PFLOP/s; the RoI stage has no matrix work to speak of"}
        rec["roofline_affinity"] = {
            "kernel": "as_cosine_shift (per iteration: similarity / assign / aggregate launches; packed final similarity)",
            "bound": "hbm", "achieved": round(gbps, 1), "peak": PEAK_HBM_GBPS, "unit": "GB/s",
            "frac": round(gbps / PEAK_HBM_GBPS, 4),
            "traffic": _static_traffic(("r06_shift_traffic.json", "r05_shift_traffic.json", "r04_shift_traffic.json", "r03_shift_traffic.json"), "per_call_bytes") if headline and imgs_per_call == 2 else None,
            "calls_timed": n_cs, "images_per_call": imgs_per_call, "ms_per_call": round(ms_cs, 4),
            "algorithmic_bytes_per_call": bytes_cs,
            "timeline": "profiles/r05_shift_timeline.md (s_memrealtime stamps inside the three iteration kernels: where each "
                        "launch's 8-12 us go)"}
        alone = block_timing.get("cosine_shift_alone")
        if alone:
            # `ms_per_call` above is measured in the timed region, where the call overlaps the images' mask-point kernels;
            # this is the same call with the device to itself (5 extra steps after the timed region)
            rec["roofline_affinity"].update(
                ms_per_call_alone=round(alone[1], 4), frac_alone=round(bytes_cs / (alone[1] * 1e-3) / 1e9 / PEAK_HBM_GBPS, 4),
                note="ms_per_call / frac: inside the timed region, sharing the device with the per-image mask-point kernels "
                     "(a step-level overlap, round 5); ms_per_call_alone / frac_alone: the same call without that overlap")
        ra = rec["roofline_affinity"]
        if ra["traffic"] is not None:
            # the same call priced by the bytes the counters saw (the kernels skip out-of-box patches, which the SURVEY 8d
            # formula counts): the honest HBM fraction, next to the algorithmic one
            cb = ra["traffic"]["bytes"]
            ra["frac_counter_bytes"] = round(cb / (ms_cs * 1e-3) / 1e9 / PEAK_HBM_GBPS, 4)
            ra["counter_over_algorithmic"] = round(cb / bytes_cs, 3)
        try:      # the dependent-chain floor of 16 launches of this grid size (tools/experiments/chain_floor.hip, this round)
            cf_name = next(n for n in ("r06_chain_floor.json", "r05_chain_floor.json", "r04_chain_floor.json") if os.path.exists(os.path.join(ROOT, "profiles", n)))
            with open(os.path.join(ROOT, "profiles", cf_name)) as f:
                cf = json.load(f)
            ra["dependent_chain_floor"] = {
                "us_16_launches_3_hops": cf["us_per_chain_by_hops"]["3"], "us_16_empty_launches": cf["us_per_chain_by_hops"]["0"],
                "us_per_dependent_hop": cf["us_per_dependent_hop"], "source": f"profiles/{cf_name} (micro-benchmark, chain queued behind a blocker so "
                "the host's launch rate does not enter: 16 dependent launches of 126 workgroups, each thread walking 3 dependent "
                "cache-resident loads) -- the launch boundaries explain ~1/6 of the call; the rest is the latency chains INSIDE "
                "the 16 kernels (operands -> MFMA -> reductions, ~8-12 us each on a quarter-full chip)"}
        except (OSError, KeyError, ValueError, StopIteration):
            pass
        # the same step on the path that meets north_star's 1e-3 (compute_dtype=float32: exact-fp32 MFMA kernels,
        # tests/test_gpu_backbone_fullsize.py); the headline is the bf16 path BASELINE config 2 names
        if a.full and os.environ.get("AS_BENCH_FP32", "1") == "1":
            try:
                fstep = build(device, rng_mode, compute_dtype=torch.float32)
                with torch.no_grad():
                    for _ in range(2):
                        fstep()
                    rec["images_per_sec_fp32_parity_path"] = round(world * B * 5 / timed(fstep, ranks, 5), 3)
                del fstep
            except Exception as e:                          # noqa: BLE001
                rec["images_per_sec_fp32_parity_path"] = None
                rec["fp32_parity_path_error"] = f"{type(e).__name__}: {e}"[:200]
        # the same step with the trainable MIL head choosing the roll-out depth from RoI-aligned features (stdroi:2308-2312)
        if a.full and os.environ.get("AS_BENCH_MIL", "1") == "1":
            del step
            torch.cuda.empty_cache()
            mstep = build(device, rng_mode, mil=True)
            with torch.no_grad():
                for _ in range(2):
                    mstep()
                rec["images_per_sec_mil_selector"] = round(world * B * a.steps / timed(mstep, ranks, a.steps), 3)
            del mstep
        else:
            del step
        torch.cuda.empty_cache()

    # ---- short forward legs of the other BASELINE configurations (configs[3] ViT-L, configs[4] Swin-B), so that one
    # --full invocation times them too; the headline numbers above are not affected ----
    if a.full and a.config == "vitb" and a.other_configs:
        rec["other_configs"] = {}
        for name in [n for n in a.other_configs.split(",") if n in CONFIGS and n != "vitb"]:
            try:
                CFG.clear()
                CFG.update(CONFIGS[name])
                ostep = build(device, rng_mode)
                ovit = CFG["backbone"] == "vit"
                with torch.no_grad():
                    for _ in range(2):
                        ostep()
                    ops.enable_timing(["sdpa_fwd", "cosine_shift"] if ovit else ["window_attn_fwd"])
                    o_steps = max(3, a.steps // 4)
                    t_o = timed(ostep, ranks, o_steps)
                ot = ops.collect_timing()
                ops.disable_timing()
                leg = {"workload": CFG["workload"], "images_per_sec": round(world * CFG["batch"] * o_steps / t_o, 3),
                       "ms_per_step": round(t_o / o_steps * 1e3, 3), "steps": o_steps, "warmup": 2}
                if ovit and "sdpa_fwd" in ot:
                    No, ho = 1 + (CFG["img"] // CFG["patch"]) ** 2 + CFG["point_tokens"], CFG["heads"]
                    fl = 4.0 * CFG["batch"] * ho * No * No * 64
                    leg["sdpa_fwd"] = {"ms_per_launch": round(ot["sdpa_fwd"][1], 4), "tflops": round(fl / ot["sdpa_fwd"][1] / 1e9, 1),
                                       "frac": round(fl / (ot["sdpa_fwd"][1] * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4)}
                if ovit and "cosine_shift" in ot:            # the affinity call at this config's G (7 objects, 80 x 80 patches)
                    n_o, ms_o = ot["cosine_shift"]
                    Npo, Co, So, Go = (CFG["img"] // CFG["patch"]) ** 2, CFG["embed_dim"], CFG["n_shift"], CFG["objects"]
                    ipc = max(1, round(CFG["batch"] * o_steps / max(n_o, 1)))
                    by_o = ipc * ((2 * So + 1) * Npo * Co * 4 + Go * 20 * Npo * 4)
                    leg["roofline_affinity"] = {"bound": "hbm", "achieved": round(by_o / (ms_o * 1e-3) / 1e9, 1), "peak": PEAK_HBM_GBPS,
                                                "unit": "GB/s", "frac": round(by_o / (ms_o * 1e-3) / 1e9 / PEAK_HBM_GBPS, 4),
                                                "ms_per_call": round(ms_o, 4), "objects_per_image": Go, "images_per_call": ipc,
                                                "algorithmic_bytes_per_call": by_o}
                if not ovit and "window_attn_fwd" in ot:
                    _, by = ot.get("window_attn_fwd:bytes", (0, float("nan")))
                    leg["window_attn_fwd"] = {"ms_per_launch": round(ot["window_attn_fwd"][1], 4),
                                              "gbps": round(by / (ot["window_attn_fwd"][1] * 1e-3) / 1e9, 1)}
                rec["other_configs"][name] = leg
                del ostep
            except Exception as e:                          # noqa: BLE001 -- never lose the headline to a side leg
                rec["other_configs"][name] = {"error": f"{type(e).__name__}: {e}"[:300]}
            torch.cuda.empty_cache()
        CFG.clear()
        CFG.update(CONFIGS[a.config])

    emitted = threading.Event()

    def emit():
        if emitted.is_set():
            return
        emitted.set()
        if rank == 0:
            os.write(real_stdout, (json.dumps(rec) + "\n").encode())

    # ---- the DDP training step (--full): default at N > 1 (that is where RCCL over xGMI runs), optional at N = 1 ----
    if a.full and vit and a.train_steps > 0:
        def give_up():
            rec["train"] = {"error": f"training leg did not finish within {a.train_timeout:.0f}s (watchdog)"}
            emit()
            os._exit(0)

        dog = threading.Timer(a.train_timeout, give_up)
        dog.daemon = True
        dog.start()
        try:
            # N = 1: the leg runs through a REAL one-rank process group (dist.Ranks(force=True): RCCL on this GPU), so the
            # bucket copies, the hook-launched all-reduces, finish() and the write-back are the code that N > 1 runs;
            # AS_FORCE_DIST=0 (or an RCCL that does not come up) falls back to the group-less step, and says so
            tranks, forced = ranks, None
            if world == 1 and os.environ.get("AS_FORCE_DIST", "1") == "1":
                try:
                    tranks = Ranks(device=device, force=True)
                    tstep = build(device, rng_mode, train=True, ranks=tranks)
                    logs = tstep()
                    forced = "one-rank process group (" + str(tranks.dist.get_backend_config()) + ")"
                except Exception as e:                      # noqa: BLE001
                    forced = f"one-rank group failed ({type(e).__name__}: {e})"[:200] + "; ran without a group"
                    tranks.close() if tranks is not ranks else None
                    tranks = ranks
                    tstep = build(device, rng_mode, train=True, ranks=ranks)
            else:
                tstep = build(device, rng_mode, train=True, ranks=ranks)
            for _ in range(2):
                logs = tstep()
            ops.enable_timing(["attn_bwd"])
            del tstep.finish_events[:]
            spread = {}
            t_train = timed(tstep, ranks, a.train_steps, per_rank=spread)
            ttiming = ops.collect_timing()
            ops.disable_timing()
            n_bwd, ms_bwd = ttiming.get("attn_bwd", (0, float("nan")))
            torch.cuda.synchronize()
            fin_ms = [e0.elapsed_time(e1) for e0, e1 in tstep.finish_events]
            red = tstep.reducer
            comm = {"group": forced or (f"{world} ranks" if world > 1 else "none"), "state_broadcasts": red.broadcasts,
                    "buckets": len(red.buckets), "bucket_bytes": [int(b["flat"].numel() * b["flat"].element_size()) for b in red.buckets],
                    "comm_dtype": str(red.comm_dtype).replace("torch.", ""),
                    # device time of reducer.finish() on the compute stream: what of the gradient all-reduce is NOT hidden
                    # under the backward (waits for the in-flight buckets + averaging / write-back), max over ranks
                    "finish_ms_per_step": round(ranks.max_over_ranks(sum(fin_ms) / max(len(fin_ms), 1)), 4)}
            # the reference's schedule: update_interval=2 (run_train.py:13) -- two micro-batches per optimizer step, one
            # all-reduce; grad_clip is None in configs/mae/attnshift_voc12aug.py:269 and stays None
            accum = None
            if a.train_accum > 1:
                astep = lambda: tstep(update_interval=a.train_accum)
                astep()
                del tstep.finish_events[:]
                n_opt = max(1, a.train_steps // a.train_accum)
                aspread = {}
                t_acc = timed(astep, ranks, n_opt, per_rank=aspread)
                torch.cuda.synchronize()
                fin2 = [e0.elapsed_time(e1) for e0, e1 in tstep.finish_events]
                accum = {"update_interval": a.train_accum, "optimizer_steps": n_opt,
                         "images_per_sec": round(world * B * a.train_accum * n_opt / t_acc, 3),
                         "ms_per_optimizer_step": round(t_acc / n_opt * 1e3, 3),
                         "finish_ms_per_step": round(ranks.max_over_ranks(sum(fin2) / max(len(fin2), 1)), 4), "per_rank": aspread}
            rec["train"] = {"images_per_sec": round(world * B * a.train_steps / t_train, 3),
                            "ms_per_step": round(t_train / a.train_steps * 1e3, 3), "steps": a.train_steps,
                            "per_rank": spread, "allreduce": comm, "accumulation": accum,
                            "attn_bwd_ms_per_layer": round(ms_bwd, 4), "attn_bwd_launches_timed": n_bwd,
                            "losses": {k: round(v, 4) for k, v in logs.items()},
                            "what": "backbone fwd (autograd, HIP attention fwd) + no-grad attention shift + RoI-head losses "
                                    "(MIL, point tokens, box, point-supervised mask; 512 sampled RoIs/img of 1000 seeded "
                                    "proposals) + bwd (HIP attention bwd) + bucketed RCCL grad all-reduce overlapped with bwd "
                                    "+ fused scalar-loss all-reduce + fused AdamW; batch " + str(B) + "/GPU"}
        except Exception as e:                              # noqa: BLE001 -- the headline must still be printed
            rec["train"] = {"error": f"{type(e).__name__}: {e}"[:300]}
        dog.cancel()
        try:
            if tranks is not ranks:
                tranks.close()
        except Exception:                                   # noqa: BLE001
            pass

    if a.full and rank == 0 and world == 1 and a.config == "vitb" and not a.no_cpu_baseline and not emitted.is_set():
        rec["cpu_baseline"] = cpu_baseline()
    emit()
    ranks.close()


if __name__ == "__main__":
    main()
