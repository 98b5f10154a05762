"""Parity of the HIP kernels (through the C ABI) against the CPU oracle and the golden vectors.

Run on the MI355X box:  python -m pytest tests -m gpu -x -q
Tolerances (stated per test): fp32 path 1e-3 relative or tighter; bf16 path compared with the fp32
oracle evaluated on bf16-rounded operands, max error <= 2e-2 of the output range; every integer
output (labels, assignments, boxes in pixel units) bit-exact.
"""
import numpy as np
import pytest
import torch

import attnshift_oracle as O
from helpers import assert_close, assert_equal, shift_case_inputs, t

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def ops():
    from attentionshift_amd import ops as _ops
    _ops._lib.load()          # fail loudly if the library is not built
    return _ops


def dev(x):
    return x.cuda().contiguous()


def rel_to_range(ref, got):
    ref, got = ref.double().cpu(), got.double().cpu()
    scale = ref.abs().max().item() + 1e-30
    err = (ref - got).abs()
    return err.max().item() / scale, err.mean().item() / scale


# ------------------------------------------------------------------------------------------------
# Part A
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(300, 192, 192), (129, 576, 64), (1000, 256, 768)])
@pytest.mark.parametrize("act", ["none", "gelu", "relu"])
def test_linear_f32(ops, M, N, K, act):
    g = torch.Generator().manual_seed(M + N + K)
    x, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.1, torch.randn(N, generator=g)
    ref = torch.nn.functional.linear(x, w, b)
    if act == "gelu":
        ref = torch.nn.functional.gelu(ref)
    if act == "relu":
        ref = torch.relu(ref)
    got = ops.linear(dev(x), dev(w), dev(b), act=act)
    assert_close(ref, got, 1e-4, 1e-4, f"linear f32 {M}x{N}x{K} {act}")


@pytest.mark.parametrize("M,N,K", [(8394, 3072, 768), (8394, 768, 3072), (4197, 768, 768), (8394, 3080, 768), (8394, 1000, 4096)])
@pytest.mark.parametrize("act", ["none", "gelu", "relu"])
def test_linear_bf16_backbone_shapes(ops, M, N, K, act):
    """as_linear_fwd in plain-linear mode on the shapes the ViT-B blocks launch (fc1 / fc2 / proj at 2 x 4197 tokens):
    fc2 / proj pick the 256 x 128 tile, fc1 (N = 3072) the 256 x 256 one (csrc/gemm.hip launch_gemm_glds; M = 513 below
    always gets the 128 x 128 one), ragged in M (8394 = 32 * 256 + 202); the last two shapes are ragged in N on the
    256 x 256 tile (3080 = 12 * 256 + 8, 1000 = 3 * 256 + 232; the second is ViT-L's fc2 depth).  vs F.linear (+ exact erf GELU) in fp32 on the same bf16-rounded operands."""
    g = torch.Generator().manual_seed(M + N)
    x = torch.randn(M, K, generator=g).bfloat16()
    w = (torch.randn(N, K, generator=g) * K ** -0.5).bfloat16()
    b = torch.randn(N, generator=g)
    ref = torch.nn.functional.linear(x.float(), w.float(), b)
    if act == "gelu":
        ref = torch.nn.functional.gelu(ref)
    if act == "relu":
        ref = torch.relu(ref)
    got = ops.linear(dev(x), dev(w), dev(b), act=act).float()
    mx, mean = rel_to_range(ref, got)
    assert mx < 1e-2 and mean < 2e-3, (mx, mean)      # output rounding to bf16 dominates


@pytest.mark.parametrize("M,N,K", [(8394, 3072, 768), (8394, 768, 3072), (8394, 768, 768), (8192, 768, 768), (6501, 4096, 1024),
                                   (6501, 1024, 4096), (5000, 1000, 1536), (8394, 3080, 768)])
@pytest.mark.parametrize("act", ["none", "gelu"])
def test_linear_stream_k_matches_the_plain_grid_and_fp32(ops, monkeypatch, M, N, K, act):
    """as_linear_sk_fwd (every workgroup the same number of K steps, tiles finished by their last-arriving piece) against
    fp32 F.linear on the same bf16 operands, against as_linear_fwd (one bf16 rounding apart at most: the pieces are summed in
    fp32 before the single rounding), bitwise reproducible call after call, and unaffected by what the previous call -- other
    operands, another shape -- left in the shared workspace."""
    lib = ops._lib.load()
    assert lib.as_linear_sk_workspace_bytes(M, N, K) == 0, "the schedule is off by default (measured slower, csrc/gemm.hip sk_plan)"
    monkeypatch.setenv("AS_GEMM_SK", "1")
    nb = lib.as_linear_sk_workspace_bytes(M, N, K)
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).bfloat16()
    w = (torch.randn(N, K, generator=g) * K ** -0.5).bfloat16()
    b = torch.randn(N, generator=g)
    ref = torch.nn.functional.linear(x.float(), w.float(), b)
    if act == "gelu":
        ref = torch.nn.functional.gelu(ref)
    xd, wd, bd = dev(x), dev(w), dev(b)
    code = 1 if act == "gelu" else 0
    st = torch.cuda.current_stream().cuda_stream
    ws = torch.full((max(nb, 16),), 0xAB, dtype=torch.uint8).cuda()                 # garbage in the partial tiles
    plain = torch.empty(M, N, dtype=torch.bfloat16).cuda()
    assert lib.as_linear_fwd(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), plain.data_ptr(), M, N, K, 1, code, st) == 0
    outs = []
    for _ in range(3):
        o = torch.empty(M, N, dtype=torch.bfloat16).cuda()
        assert lib.as_linear_sk_fwd(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), o.data_ptr(), M, N, K, 1, code, ws.data_ptr(),
                                    ws.numel(), st) == 0
        outs.append(o)
    mx, mean = rel_to_range(ref, outs[0].float())
    assert mx < 1e-2 and mean < 2e-3, (mx, mean, nb)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), "stream-K must be bitwise reproducible"
    rng = float(plain.float().abs().max())
    assert float((outs[0].float() - plain.float()).abs().max()) <= 8e-3 * rng      # one bf16 ulp of the largest values
    # different operands through the SAME workspace, then the first operands again
    x2 = dev((torch.randn(M, K, generator=g) * 2).bfloat16())
    o2 = torch.empty(M, N, dtype=torch.bfloat16).cuda()
    assert lib.as_linear_sk_fwd(x2.data_ptr(), wd.data_ptr(), bd.data_ptr(), o2.data_ptr(), M, N, K, 1, code, ws.data_ptr(),
                                ws.numel(), st) == 0
    o3 = torch.empty(M, N, dtype=torch.bfloat16).cuda()
    assert lib.as_linear_sk_fwd(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), o3.data_ptr(), M, N, K, 1, code, ws.data_ptr(),
                                ws.numel(), st) == 0
    assert torch.equal(o3, outs[0])
    print(f"[stream-K] {M}x{N}x{K}: workspace {nb} bytes ({'stream-K' if nb else 'plain grid'})")


@pytest.mark.parametrize("M,N,K", [(768, 768, 8448), (2304, 768, 8448), (3072, 768, 8448), (200, 132, 96), (130, 64, 4096)])
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
def test_linear_splitk_matches_fp32_matmul(ops, M, N, K, out_dtype):
    """as_linear_splitk_fwd (the weight-gradient GEMM form: tokens as K, contraction split over workgroups, fixed-order fp32
    partials) vs an fp32 matmul of the same bf16 operands; run twice: bitwise equal (no atomics)."""
    g = torch.Generator().manual_seed(M + N + K)
    x = (torch.randn(M, K, generator=g) * 0.5).bfloat16()
    w = (torch.randn(N, K, generator=g) * 0.5).bfloat16()
    ref = x.double() @ w.double().t()
    got = ops.linear_splitk(dev(x), dev(w), out_dtype)
    assert got.dtype == out_dtype and got.shape == (M, N)
    mx, mean = rel_to_range(ref, got.float())
    assert mx < (1e-2 if out_dtype == torch.bfloat16 else 2e-5) and mean < 2e-3, (mx, mean)
    assert torch.equal(got, ops.linear_splitk(dev(x), dev(w), out_dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,w_dtype", [(8394, 3072, 768, torch.bfloat16), (8394, 768, 3072, torch.bfloat16),
                                           (51200, 1024, 256, torch.float32), (50176, 256, 768, torch.float32),
                                           (1000, 96, 36, torch.float32)])
def test_linear_autograd_fn_matches_fp64_autograd(ops, M, N, K, w_dtype):
    """autograd.LinearFn (as_linear_fwd forward, as_linear_bwd backward: dx on the forward kernel, split-K dW, column-sum
    db) vs fp64 autograd of the same bf16-rounded operands; shapes: the backbone MLP and the MAE heads' layers (rows of
    50 k tokens, fp32 master weights) and a small ragged one.  Run twice: bitwise equal gradients (no atomics)."""
    from attentionshift_amd import autograd as AG
    g = torch.Generator().manual_seed(M + N + K)
    x = (torch.randn(M, K, generator=g) * 0.5).bfloat16()
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(w_dtype)
    b = torch.randn(N, generator=g)
    dy = (torch.randn(M, N, generator=g) * 0.1).bfloat16()
    if K % 32:                                              # sizes the kernels do not take are refused by the predicate
        assert not AG.linear_applies(dev(x), dev(w))
        return
    with torch.enable_grad():
        xr, wr, br = x.double().requires_grad_(True), w.bfloat16().double().requires_grad_(True), b.double().requires_grad_(True)
        ref = torch.nn.functional.linear(xr, wr, br)
        ref.backward(dy.double())

        def run():
            xd, wd, bd = dev(x).requires_grad_(True), dev(w).requires_grad_(True), dev(b).requires_grad_(True)
            out = AG.linear(xd, wd, bd)
            out.backward(dev(dy))
            return out.detach(), xd.grad, wd.grad, bd.grad

        out, dx, dw, db = run()
    assert out.dtype == torch.bfloat16 and dx.dtype == torch.bfloat16 and dw.dtype == w_dtype and db.dtype == torch.float32
    for name, got, want, tol in (("out", out, ref.detach(), 1e-2), ("dx", dx, xr.grad, 1e-2),
                                 ("dw", dw, wr.grad, 1e-2 if w_dtype == torch.bfloat16 else 1e-4), ("db", db, br.grad, 1e-4)):
        mx, mean = rel_to_range(want, got.float())
        assert mx < tol and mean < tol / 5, (name, mx, mean)
    with torch.enable_grad():
        again = run()
    assert all(torch.equal(a, b_) for a, b_ in zip((out, dx, dw, db), again))


_TILE_SCRIPT = """
import sys, torch
sys.path.insert(0, %r)
from attentionshift_amd import ops
torch.manual_seed(0)
worst = 0.0
for (M, N, K, act) in [(300, 520, 64, "none"), (300, 520, 128, "gelu"), (1000, 264, 192, "none"), (8394, 768, 768, "none"),
                       (2049, 3072, 768, "gelu"), (257, 1000, 1024, "none")]:
    x = torch.randn(M, K).bfloat16(); w = (torch.randn(N, K) * K ** -0.5).bfloat16(); b = torch.randn(N)
    ref = torch.nn.functional.linear(x.float(), w.float(), b)
    if act == "gelu":
        ref = torch.nn.functional.gelu(ref)
    got = ops.linear(x.cuda(), w.cuda(), b.cuda(), act=act).float().cpu()
    worst = max(worst, float((ref - got).abs().max() / ref.abs().max()))
print("WORST", worst)
"""


@pytest.mark.parametrize("tile", ["short", "tall", "tall64", "wide64"])
def test_linear_bf16_every_tile_shape_forced(tile):
    """Every instantiation of gemm_glds_kernel (csrc/gemm.hip launch_gemm_glds) on shapes that are ragged in M and N, with
    one, two and many K stages, through the same C entry point: AS_GEMM_TILE is read once per process, so each tile runs
    in its own interpreter.  (K = 64 / 128: single- and two-stage pipelines of the K-step-64 tiles.)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, AS_GEMM_TILE=tile)
    out = subprocess.run([sys.executable, "-c", _TILE_SCRIPT % root], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    worst = float(out.stdout.strip().split("WORST")[-1])
    assert worst < 1e-2, (tile, worst)


def test_linear_bf16(ops):
    g = torch.Generator().manual_seed(1)
    x, w, b = torch.randn(513, 768, generator=g), torch.randn(384, 768, generator=g) * 0.05, torch.randn(384, generator=g)
    xb, wb = x.bfloat16(), w.bfloat16()
    ref = torch.nn.functional.linear(xb.float(), wb.float(), b)
    got = ops.linear(dev(xb), dev(wb), dev(b)).float()
    mx, mean = rel_to_range(ref, got)
    assert mx < 1e-2 and mean < 2e-3, (mx, mean)      # output rounding to bf16 dominates


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,N", [(2, 150), (3, 421), (2, 4197), (1, 517)])
def test_qkv_layout(ops, dtype, B, N):
    """q / k / V^T workspaces of as_qkv_fwd.  The bf16 V^T tiles are transposed through LDS with the staging columns shifted by
    (first token's index in its image) % 8: images of 421 / 4197 tokens start at every residue, (2, 150) and (3, 421) have
    tiles that straddle an image boundary (direct path), and the padded columns [N, Npad) must stay untouched."""
    h = 3
    D = 64 * h
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, N, D, generator=g).to(dtype)
    w = (torch.randn(3 * D, D, generator=g) * 0.05).to(dtype)
    b = torch.randn(3 * D, generator=g)
    ref = torch.nn.functional.linear(x.float(), w.float(), b).reshape(B, N, 3, h, 64).permute(2, 0, 3, 1, 4)
    q, k, vt = ops.qkv_fwd(dev(x), dev(w), dev(b), h)
    tol = 1e-4 if dtype == torch.float32 else 2e-2
    if dtype == torch.bfloat16:                            # a second call into poisoned workspaces: only [.., :N] is written
        from attentionshift_amd import _lib
        lib = _lib.load()
        q2, k2, vt2 = (torch.full_like(t_, 7.0) for t_ in (q, k, vt))
        xd, wd, bd = dev(x), dev(w), dev(b)
        assert lib.as_qkv_fwd(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), q2.data_ptr(), k2.data_ptr(), vt2.data_ptr(), B, N, D, h,
                              1, torch.cuda.current_stream().cuda_stream) == 0
        assert torch.equal(vt2[:, :, :, :N], vt[:, :, :, :N]) and (vt2[:, :, :, N:] == 7.0).all(), "V^T: stray or missing writes"
    # q is stored pre-scaled by log2(e) / 8 (one rounding, from the fp32 accumulator)
    assert_close(ref[0] * ops.QSCALE, ops.q_from_fragment_major(q)[:, :, :N].float(), tol, tol, "q (fragment-major, pre-scaled)")
    assert_close(ref[1], k[:, :, :N].float(), tol, tol, "k")
    assert_close(ref[2].transpose(-1, -2), vt[:, :, :, :N].float(), tol, tol, "v^T")


def _attn_inputs(B, N, h, seed, scale=1.0):
    D = 64 * h
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, D, generator=g)
    wqkv = torch.randn(3 * D, D, generator=g) * (scale / D ** 0.5)
    bqkv = torch.randn(3 * D, generator=g) * 0.1
    wproj = torch.randn(D, D, generator=g) / D ** 0.5
    bproj = torch.randn(D, generator=g) * 0.1
    return x, wqkv, bqkv, wproj, bproj


@pytest.mark.parametrize("B,N,h", [(2, 297, 3), (1, 64, 1), (1, 1000, 2), (1, 4197, 2), (1, 6501, 1)])
def test_attention_f32_matches_oracle(ops, B, N, h):
    """fp32 MFMA path vs Attention.forward restated in the oracle; tolerance 1e-4 of the range
    (north_star asks 1e-3)."""
    x, wqkv, bqkv, wproj, bproj = _attn_inputs(B, N, h, 10 + N, scale=3.0)
    ref, p = O.attention(x, wqkv, bqkv, wproj, bproj, h)
    out, st = ops.attention_fwd(dev(x), dev(wqkv), dev(bqkv), dev(wproj), dev(bproj), h)
    mx, _ = rel_to_range(ref, out)
    assert mx < 1e-4, mx
    # log-sum-exp and recomputed head-mean rows
    qkv = torch.nn.functional.linear(x, wqkv, bqkv).reshape(B, N, 3, h, 64).permute(2, 0, 3, 1, 4)
    lse_ref = torch.logsumexp((qkv[0] @ qkv[1].transpose(-1, -2)) * 0.125, dim=-1)
    assert_close(lse_ref, st.lse, 1e-5, 1e-4, "lse")
    rows = ops.attn_mean_rows(st, max(N - 100, 0), min(100, N))
    assert_close(p.mean(1)[:, max(N - 100, 0):], rows, 1e-3, 1e-7, "head-mean rows")


@pytest.mark.parametrize("B,N,h", [(2, 297, 3), (1, 4197, 2)])
def test_attention_bf16_matches_oracle(ops, B, N, h):
    """bf16 operands / fp32 accumulate vs the fp32 oracle on bf16-rounded x and W: mean error <= 3e-3 of the output range,
    max <= 3e-2.  (The max is set by the bf16 rounding of q and k themselves -- the oracle keeps them in fp32 -- on rows
    where two keys nearly tie at scale-3 logits: 1.9e-2 .. 2.2e-2 across kernel variants and roundings of q.)"""
    x, wqkv, bqkv, wproj, bproj = _attn_inputs(B, N, h, 20 + N, scale=3.0)
    xb, wq, wp = x.bfloat16(), wqkv.bfloat16(), wproj.bfloat16()
    ref, _ = O.attention(xb.float(), wq.float(), bqkv, wp.float(), bproj, h)
    out, st = ops.attention_fwd(dev(xb), dev(wq), dev(bqkv), dev(wp), dev(bproj), h)
    mx, mean = rel_to_range(ref, out.float())
    assert mx < 3e-2 and mean < 3e-3, (mx, mean)


def test_sdpa_spike_row_forces_rescale(ops):
    """Online-softmax rescale branch: one key dominates a query late in the sequence (guide T13)."""
    B, N, h = 1, 700, 1
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(B, h, N, 64, generator=g) for _ in range(3))
    k[0, 0, 650] = q[0, 0, 5] * 4.0        # huge logit for query 5 at the 11th KV tile
    Np_ = ops.npad(N)
    qp = torch.zeros(B, h, Np_, 64); kp = torch.zeros(B, h, Np_, 64); vtp = torch.zeros(B, h, 64, Np_)
    qs = q * ops.QSCALE                    # the stored, pre-scaled q'; the reference uses exactly these values
    qp[:, :, :N], kp[:, :, :N], vtp[:, :, :, :N] = qs, k, v.transpose(-1, -2)
    o, lse = ops.sdpa_fwd(ops.q_to_fragment_major(dev(qp)), dev(kp), dev(vtp), N)
    p = ((qs @ k.transpose(-1, -2)) * ops.LN2).softmax(-1)
    ref = (p @ v).transpose(1, 2).reshape(B, N, 64)
    mx, _ = rel_to_range(ref, o)
    assert mx < 1e-4, mx


@pytest.mark.parametrize("tail,N", [("0", 1000), ("1", 1000), ("1", 100), ("1", 1153)])
def test_sdpa_bf16_deferred_max_and_spikes(ops, monkeypatch, tail, N):
    """bf16 LDS-DMA kernel: the re-referencing branch of the softmax must be taken for spiked rows and skipped for the
    rest, with results matching the fp32 oracle on the same bf16-rounded operands (max error <= 2e-2 of the range).
    Spikes at several tiles, one of them in the ragged last tile.  tail=1 forces the last q-tile of every (image, head)
    through the key-split tail kernel (N=100: every row; N=1153: a single row in the tail)."""
    monkeypatch.setenv("AS_SDPA_TAIL", tail)
    B, h = 1, 2
    g = torch.Generator().manual_seed(31)
    q, k, v = (torch.randn(B, h, N, 64, generator=g) for _ in range(3))
    for (qi, ki, s) in ((5, 650, 6.0), (77, 130, 9.0), (400, 999, 12.0), (401, 3, 5.0), (N - 3, N - 1, 9.0), (N - 2, 1, 7.0)):
        qi, ki = qi % N, ki % N
        k[0, 0, ki] = q[0, 0, qi] * s / 8.0
        k[0, 1, ki] = q[0, 1, qi] * s / 8.0
    qb, kb, vb = (q * ops.QSCALE).bfloat16(), k.bfloat16(), v.bfloat16()     # qb = the stored, pre-scaled q'
    Np_ = ops.npad(N)
    qp = torch.zeros(B, h, Np_, 64, dtype=torch.bfloat16); kp = torch.zeros_like(qp)
    vtp = torch.full((B, h, 64, Np_), float("nan"), dtype=torch.bfloat16)        # padded keys hold garbage on purpose
    qp[:, :, :N], kp[:, :, :N], vtp[:, :, :, :N] = qb, kb, vb.transpose(-1, -2)
    kp[:, :, N:] = float("nan")
    o, lse = ops.sdpa_fwd(ops.q_to_fragment_major(dev(qp)), dev(kp), dev(vtp), N)
    s_ = (qb.float() @ kb.float().transpose(-1, -2)) * ops.LN2
    ref = (s_.softmax(-1) @ vb.float()).transpose(1, 2).reshape(B, N, h * 64)
    mx, mean = rel_to_range(ref, o.float())
    assert mx < 2e-2 and mean < 3e-3, (mx, mean)
    assert_close(torch.logsumexp(s_, dim=-1), lse, 1e-4, 1e-3, "lse (bf16 path)")
    assert torch.isfinite(o.float()).all()


@pytest.mark.parametrize("impl", ["0", "1", "2", "3", "4", "5", "6", "7"])
@pytest.mark.parametrize("tail,N", [("0", 1000), ("1", 1153), ("1", 100)])
def test_sdpa_bf16_out_of_range_logits_take_the_exact_pass(ops, monkeypatch, impl, tail, N):
    """Rows the reference-free first pass (sdpa_fwd_pipe_kernel MODE 1: P = exp2 of the raw base-2 logit) cannot represent
    -- a logit of +140 (exp overflows fp32), a row whose logits all sit near -120 (every weight underflows to 0), and a row
    mixing -150 .. +150 -- must come out of the exact (row-max referenced) pass the workgroup then runs; every kernel
    variant behind as_sdpa_fwd is held to the same fp32 oracle on the same bf16 operands, the key-split tail included."""
    monkeypatch.setenv("AS_SDPA_TAIL", tail)
    monkeypatch.setenv("AS_SDPA_IMPL", impl)
    if impl == "6":                        # stream-K on a small shape: 5 workgroups cut the 8 units (2 heads x 4 q-tiles at
        monkeypatch.setenv("AS_SDPA_SK_GRID", "5")   # N = 1000) into uneven pieces; the exact pass then runs per PIECE
    B, h = 1, 2
    g = torch.Generator().manual_seed(131)
    q, k, v = (torch.randn(B, h, N, 64, generator=g) for _ in range(3))
    u = torch.nn.functional.normalize(torch.randn(64, generator=g), dim=0)
    # head 0: overflow -- logit 40*28/8 = +140 for one (row, key); -150 next to +150 in another row
    q[0, 0, 7 % N] = u * 40.0;  k[0, 0, 650 % N] = u * 28.0
    q[0, 0, 300 % N] = u * 40.0; k[0, 0, 5] = -u * 30.0; k[0, 0, 6] = u * 30.0
    # head 1: underflow -- every key carries -32 u, so row N-2 (q = 30 u) sees logits of -120 +- 4 and nothing else
    k[0, 1] -= 32.0 * u
    q[0, 1, N - 2] = u * 30.0
    qb, kb, vb = (q * ops.QSCALE).bfloat16(), k.bfloat16(), v.bfloat16()
    Np_ = ops.npad(N)
    qp = torch.zeros(B, h, Np_, 64, dtype=torch.bfloat16); kp = torch.zeros_like(qp)
    vtp = torch.full((B, h, 64, Np_), float("nan"), dtype=torch.bfloat16)
    qp[:, :, :N], kp[:, :, :N], vtp[:, :, :, :N] = qb, kb, vb.transpose(-1, -2)
    kp[:, :, N:] = float("nan")
    o, lse = ops.sdpa_fwd(ops.q_to_fragment_major(dev(qp)), dev(kp), dev(vtp), N)
    s_ = (qb.double() @ kb.double().transpose(-1, -2)) * ops.LN2
    assert s_.max().item() > 100 and s_.max(-1)[0].min().item() < -95, "the case must leave the fp32 exp range both ways"
    ref = (s_.softmax(-1) @ vb.double()).transpose(1, 2).reshape(B, N, h * 64).float()
    assert torch.isfinite(o.float()).all()
    mx, mean = rel_to_range(ref, o.float())
    assert mx < 2e-2 and mean < 3e-3, (mx, mean)
    assert_close(torch.logsumexp(s_, dim=-1).float(), lse, 1e-4, 2e-3, "lse")


def _sdpa_case(ops, B, h, N, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, h, N, 64, generator=g) * scale for _ in range(3))
    qb, kb, vb = (q * ops.QSCALE).bfloat16(), k.bfloat16(), v.bfloat16()
    Np_ = ops.npad(N)
    qp = torch.zeros(B, h, Np_, 64, dtype=torch.bfloat16); kp = torch.zeros_like(qp)
    vtp = torch.full((B, h, 64, Np_), float("nan"), dtype=torch.bfloat16)        # padded keys hold garbage on purpose
    qp[:, :, :N], kp[:, :, :N], vtp[:, :, :, :N] = qb, kb, vb.transpose(-1, -2)
    kp[:, :, N:] = float("nan")
    s_ = (qb.float() @ kb.float().transpose(-1, -2)) * ops.LN2
    ref = (s_.softmax(-1) @ vb.float()).transpose(1, 2).reshape(B, N, h * 64)
    return ops.q_to_fragment_major(dev(qp)), dev(kp), dev(vtp), ref, torch.logsumexp(s_, dim=-1)


@pytest.mark.parametrize("B,h,N,grid", [(1, 2, 1000, "5"), (1, 2, 1000, "24"), (2, 3, 1153, "7"), (1, 1, 2049, "16"),
                                        (1, 3, 700, "3"), (2, 12, 4197, "")])
def test_sdpa_stream_k_matches_oracle_and_the_plain_grid(ops, monkeypatch, B, h, N, grid):
    """Stream-K forward (sdpa_fwd_pipe_kernel<2, 2, 1>, AS_SDPA_IMPL=6): the flattened (q-tile, key-tile) space cut into
    equal ranges, units finished by their last-arriving piece.  Small shapes with forced grids give 1, 2, 3 and many pieces
    per unit (grid 24 on 8 units: every unit in three or more pieces; grid 3 on 9 units: workgroups spanning whole units in
    the middle of their range); the last case is BASELINE config 2 at the grid the library picks by itself.  Held to the fp32
    oracle like every other variant, to the plain 256-row grid (impl 4) within the bf16 rounding of the exchanged
    partials, bitwise reproducible call after call, and immune to what the previous call left in workspace and caches."""
    if grid:
        monkeypatch.setenv("AS_SDPA_SK_GRID", grid)
    qf, kp, vtp, ref, lse_ref = _sdpa_case(ops, B, h, N, 77 + N)
    monkeypatch.setenv("AS_SDPA_IMPL", "4")
    o4, lse4 = ops.sdpa_fwd(qf, kp, vtp, N)
    monkeypatch.setenv("AS_SDPA_IMPL", "6")
    o6, lse6 = ops.sdpa_fwd(qf, kp, vtp, N)
    assert torch.isfinite(o6.float()).all()
    mx, mean = rel_to_range(ref, o6.float())
    assert mx < 2e-2 and mean < 3e-3, (mx, mean)
    assert_close(lse_ref, lse6, 1e-4, 1e-3, "lse (stream-K)")
    rng = float(o4.float().abs().max())
    assert float((o6.float() - o4.float()).abs().max()) <= 1.2e-2 * rng       # two bf16 roundings apart at most
    assert float((lse6 - lse4).abs().max()) <= 2e-3
    # the merge happened somewhere (otherwise this test is not testing stream-K) unless the cut falls on unit boundaries
    again, lse_again = ops.sdpa_fwd(qf, kp, vtp, N)
    assert torch.equal(again, o6) and torch.equal(lse_again, lse6)            # piece-ordered merge: bitwise reproducible
    # new operands in the SAME buffers (same workspace block from the caching allocator, caches warm with the old partials)
    qf2, kp2, vtp2, ref2, lse_ref2 = _sdpa_case(ops, B, h, N, 1077 + N, scale=1.5)
    qf.copy_(qf2); kp.copy_(kp2); vtp.copy_(vtp2)
    for _ in range(3):
        o6b, lse6b = ops.sdpa_fwd(qf, kp, vtp, N)
        mx, mean = rel_to_range(ref2, o6b.float())
        assert mx < 2e-2 and mean < 3e-3, (mx, mean)
        assert_close(lse_ref2, lse6b, 1e-4, 1e-3, "lse (stream-K, second operand set)")


def _sdpa_matched_reference(qb, kb, vb):
    """Precision-matched restatement of the shipped bf16 forward (models/vision_transformer.py:79-83 at the kernel's own
    rounding points): q' = q * log2(e)/8, k, v are the bf16 VALUES the kernel reads; the base-2 logits S = q'.k and the
    weights P = 2^S are fp32; the row sum adds the fp32 weights; the P.V product takes P ROUNDED TO bf16 (the MFMA B
    operand); the output is rounded to bf16 once.  (A running-max variant scales P by a power of two that is not an
    integer power, which moves individual roundings of P by one bf16 ulp -- an O(1e-4) effect on a 4197-key average.)"""
    s2 = qb.double() @ kb.double().transpose(-1, -2)                    # exact products, fp64 sums: the fp32 MFMA sum to ~1e-7
    p = torch.exp2(s2.float())                                          # fp32 weights, no reference subtracted (MODE 1)
    l = p.double().sum(-1, keepdim=True)
    o = (p.bfloat16().double() @ vb.double()) / l
    B, h, N, _ = qb.shape
    return o.transpose(1, 2).reshape(B, N, h * 64).float().bfloat16().float()


@pytest.mark.parametrize("impl", ["", "0", "1", "2", "3", "4", "5", "6", "7"])
@pytest.mark.parametrize("N,h", [(4197, 2), (6501, 1)])
def test_sdpa_bf16_against_the_precision_matched_oracle(ops, monkeypatch, impl, N, h):
    """The bf16 kernels that the benchmark times (and every variant behind AS_SDPA_IMPL) at the ViT-B / ViT-L token counts
    against an oracle that rounds where they round: max error <= 5e-3 of the output range, mean <= 5e-4 (the fp32-softmax
    oracle of the other bf16 tests leaves the rounding of P in the error and needs 2e-2 / 3e-3)."""
    if impl:
        monkeypatch.setenv("AS_SDPA_IMPL", impl)
    else:
        monkeypatch.delenv("AS_SDPA_IMPL", raising=False)
    B = 1
    g = torch.Generator().manual_seed(4000 + N)
    # logits of standard deviation ~4 (q, k at scale 2): peaked rows, outputs of order 1 -- with unit-scale operands every
    # output is a 4197-key average of order 0.05 and ONE bf16 ulp of it is already 4e-3 of the output range
    q, k = (torch.randn(B, h, N, 64, generator=g) * 2.0 for _ in range(2))
    v = torch.randn(B, h, N, 64, generator=g)
    qb, kb, vb = (q * ops.QSCALE).bfloat16(), k.bfloat16(), v.bfloat16()
    Np_ = ops.npad(N)
    qp = torch.zeros(B, h, Np_, 64, dtype=torch.bfloat16); kp = torch.zeros_like(qp)
    vtp = torch.full((B, h, 64, Np_), float("nan"), dtype=torch.bfloat16)
    qp[:, :, :N], kp[:, :, :N], vtp[:, :, :, :N] = qb, kb, vb.transpose(-1, -2)
    kp[:, :, N:] = float("nan")
    o, lse = ops.sdpa_fwd(ops.q_to_fragment_major(dev(qp)), dev(kp), dev(vtp), N)
    ref = _sdpa_matched_reference(qb, kb, vb)
    assert ref.abs().max() > 1.0
    mx, mean = rel_to_range(ref, o.float())
    assert mx <= 5e-3 and mean <= 5e-4, (impl, N, mx, mean)
    s_ = (qb.double() @ kb.double().transpose(-1, -2)) * ops.LN2
    assert_close(torch.logsumexp(s_, dim=-1).float(), lse, 1e-4, 1e-3, "lse")


@pytest.mark.parametrize("B,h,N", [(1, 2, 1000), (2, 3, 1153), (1, 1, 513), (1, 2, 100), (2, 12, 4197)])
def test_sdpa_eight_wave_workgroups_match_oracle_and_the_plain_grid(ops, monkeypatch, B, h, N):
    """AS_SDPA_IMPL=7: the pipelined kernel on 512-row workgroups of eight waves (each K / V^T tile staged once for twice the
    queries): against the fp32 oracle and, row for row, against the 256-row grid -- the same arithmetic per wave, so bitwise
    equal outputs are expected; ragged last tiles with 1 .. 7 waves that own no query (N = 513: seven of eight)."""
    qf, kp, vtp, ref, lse_ref = _sdpa_case(ops, B, h, N, 99 + N)
    monkeypatch.setenv("AS_SDPA_IMPL", "4")
    o4, lse4 = ops.sdpa_fwd(qf, kp, vtp, N)
    monkeypatch.setenv("AS_SDPA_IMPL", "7")
    o7, lse7 = ops.sdpa_fwd(qf, kp, vtp, N)
    assert torch.isfinite(o7.float()).all()
    mx, mean = rel_to_range(ref, o7.float())
    assert mx < 2e-2 and mean < 3e-3, (mx, mean)
    assert_close(lse_ref, lse7, 1e-4, 1e-3, "lse (8 waves)")
    assert torch.equal(o7, o4) and torch.equal(lse7, lse4)


@pytest.mark.parametrize("B,H,W,C,k", [(2, 64, 64, 768, 2), (1, 12, 20, 192, 4), (2, 6, 10, 128, 2)])
def test_maxpool_nhwc_equals_max_pool2d(ops, B, H, W, C, k):
    """as_maxpool_nhwc (the FPN's stride-32 tap on the token-major layout) == nn.MaxPool2d(k, k) bit for bit, NaN included."""
    g = torch.Generator().manual_seed(H * W + C)
    x = torch.randn(B, H, W, C, generator=g)
    x[0, 1, 1, 3] = float("nan")
    ref = torch.nn.functional.max_pool2d(x.permute(0, 3, 1, 2), k, k).permute(0, 2, 3, 1)
    got = ops.maxpool_nhwc(dev(x), k).cpu()
    assert got.shape == ref.shape
    assert torch.equal(torch.nan_to_num(got, nan=-7.0), torch.nan_to_num(ref, nan=-7.0))
    # the form the backbone uses: the patch-token slice of [B, 1 + Np + T, C] -- dense images, strided batch, no copy
    tokens = torch.zeros(B, 1 + H * W + 5, C)
    tokens[:, 1:1 + H * W] = x.reshape(B, H * W, C)
    tok_dev = dev(tokens)
    view = tok_dev[:, 1:1 + H * W].reshape(B, H, W, C) if B == 1 else tok_dev[:, 1:1 + H * W].unflatten(1, (H, W))
    assert B == 1 or not view.is_contiguous()
    got2 = ops.maxpool_nhwc(view, k).cpu()
    assert torch.equal(torch.nan_to_num(got2, nan=-7.0), torch.nan_to_num(ref, nan=-7.0))


@pytest.mark.parametrize("M,D", [(297, 192), (1000, 768), (77, 1024), (5, 128)])
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-6), (torch.bfloat16, 1e-2)])
def test_add_layernorm_matches_torch(ops, dtype, tol, M, D):
    """Fused residual add + LayerNorm (Block.forward's `x = x + f(norm(x))` chain, vision_transformer.py:109-124) vs
    torch: x_new exact in fp32 (one add), y within rounding of F.layer_norm on the same x_new."""
    g = torch.Generator().manual_seed(M + D)
    x = torch.randn(2, M, D, generator=g) * 3 + 0.5
    delta = (torch.randn(2, M, D, generator=g)).to(dtype)
    gamma, beta = torch.randn(D, generator=g) * 0.2 + 1.0, torch.randn(D, generator=g) * 0.1
    x_ref = x + delta.float()
    y_ref = torch.nn.functional.layer_norm(x_ref, (D,), gamma, beta, 1e-6)
    x_new, y = ops.add_layernorm(dev(x), dev(delta), dev(gamma), dev(beta), 1e-6, dtype)
    assert_equal(x_ref, x_new, "x + delta")
    mx, _ = rel_to_range(y_ref, y.float())
    assert mx < tol, mx
    _, y0 = ops.add_layernorm(dev(x), None, dev(gamma), dev(beta), 1e-6, dtype)          # LN only
    mx, _ = rel_to_range(torch.nn.functional.layer_norm(x, (D,), gamma, beta, 1e-6), y0.float())
    assert mx < tol, mx
    x_only, none = ops.add_layernorm(dev(x), dev(delta), None, None, 0.0, dtype, want_y=False)   # add only
    assert none is None
    assert_equal(x_ref, x_only, "add only")


def test_attention_bf16_vit_large_token_count(ops):
    """BASELINE config 4 token count (ViT-L at 1280^2: N = 1 + 80*80 + 100 = 6501, 51 q-tiles, ragged last key tile)
    through the bf16 path, 4 of its 16 heads' worth of width, vs the oracle's Attention.forward."""
    B, N, h = 1, 6501, 4
    x, wqkv, bqkv, wproj, bproj = _attn_inputs(B, N, h, 17, scale=2.0)
    xd, wq, wp = x.bfloat16(), wqkv.bfloat16(), wproj.bfloat16()
    ref, p = O.attention(xd.float(), wq.float(), bqkv, wp.float(), bproj, h)
    out, st = ops.attention_fwd(dev(xd), dev(wq), dev(bqkv), dev(wp), dev(bproj), h)
    mx, mean = rel_to_range(ref, out.float())
    assert mx < 3e-2 and mean < 3e-3, (mx, mean)
    rows = ops.attn_mean_rows(st, N - 100, 100)
    mx, _ = rel_to_range(p.mean(1)[:, N - 100:], rows)
    assert mx < 3e-2, mx


@pytest.mark.parametrize("B,N,h", [(1, 297, 3), (2, 200, 2), (1, 1000, 2), (1, 64, 1), (1, 65, 2), (2, 129, 1)])
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4), (torch.bfloat16, 3e-2)])
def test_sdpa_bwd_matches_autograd(ops, dtype, tol, B, N, h):
    """Backward of A2 (autograd of vision_transformer.py:79-83): dq, dk, dv from the tile-recomputing HIP kernels vs
    torch autograd (fp64) of softmax(q k^T / 8) v on the same (dtype-rounded) operands.  Padded rows of the q/k/v^T
    workspaces hold NaN on purpose: nothing outside [0, N) may leak into a gradient.
    Tolerance: max error relative to the gradient's range; 1e-4 fp32 (north_star asks 1e-3), 3e-2 bf16."""
    g = torch.Generator().manual_seed(77 + N)
    q, k, v = (torch.randn(B, h, N, 64, generator=g) for _ in range(3))
    q = q * 1.5
    d_o = torch.randn(B, N, h * 64, generator=g)
    qd, kd, vd, dod = (q * ops.QSCALE).to(dtype), k.to(dtype), v.to(dtype), d_o.to(dtype)     # qd = the stored q'
    # fp64 autograd reference on the rounded operands; the gradient is taken w.r.t. the UNSCALED q = q' / QSCALE
    with torch.enable_grad():
        q64, k64, v64 = (t.double().requires_grad_(True) for t in (qd.double() / ops.QSCALE, kd, vd))
        o64 = (torch.softmax(q64 @ k64.transpose(-1, -2) * 0.125, -1) @ v64).transpose(1, 2).reshape(B, N, h * 64)
        o64.backward(dod.double())
    ref = torch.stack([q64.grad, k64.grad, v64.grad], 0).permute(1, 3, 0, 2, 4).reshape(B, N, 3 * h * 64).float()
    Np_ = ops.npad(N)
    nan = float("nan")
    qp = torch.full((B, h, Np_, 64), nan, dtype=dtype); kp = torch.full_like(qp, nan)
    vtp = torch.full((B, h, 64, Np_), nan, dtype=dtype)
    qp[:, :, :N], kp[:, :, :N], vtp[:, :, :, :N] = qd, kd, vd.transpose(-1, -2)
    qf, kdev, vtdev = ops.q_to_fragment_major(dev(qp)), dev(kp), dev(vtp)
    o, lse = ops.sdpa_fwd(qf, kdev, vtdev, N)
    dqkv = ops.sdpa_bwd(qf, kdev, vtdev, o, dev(dod), lse, N)
    assert torch.isfinite(dqkv.float()).all()
    got = dqkv.float().cpu().reshape(B, N, 3, h * 64)
    refr = ref.reshape(B, N, 3, h * 64)
    for i, name in enumerate(("dq", "dk", "dv")):
        mx, mean = rel_to_range(refr[:, :, i], got[:, :, i])
        assert mx < tol, (name, mx, mean)


def test_sdpa_bwd_full_size_properties(ops):
    """BASELINE config 2 shape (B=2, h=12, N=4197, bf16), where an fp64 autograd reference is too big to run in seconds:
    size-independent properties of the backward.
      * determinism: two runs are bitwise equal (no atomics, fixed summation order);
      * linearity in dO: scaling dO by 2 (exact in bf16) scales dq, dk, dv by exactly 2;
      * dO = 1: dV[key, d] = sum_q P[q, key], so summing dV over keys gives N per (image, head, d) (rows of P sum to 1);
      * <q, dq> = <k, dk> per (image, head) (both are scale * sum_ij dS_ij S_ij)."""
    B, N, h = 2, 4197, 12
    g = torch.Generator().manual_seed(9)
    x, wqkv, bqkv, _, _ = _attn_inputs(B, N, h, 123, scale=2.0)
    q, k, vt = ops.qkv_fwd(dev(x.bfloat16()), dev(wqkv.bfloat16()), dev(bqkv), h)
    o, lse = ops.sdpa_fwd(q, k, vt, N)
    d_o = dev(torch.randn(B, N, 64 * h, generator=g).bfloat16())
    g1 = ops.sdpa_bwd(q, k, vt, o, d_o, lse, N)
    g2 = ops.sdpa_bwd(q, k, vt, o, d_o, lse, N)
    assert torch.equal(g1, g2)
    assert torch.isfinite(g1.float()).all()
    g3 = ops.sdpa_bwd(q, k, vt, o, d_o * 2, lse, N)
    assert torch.equal(g3.float(), g1.float() * 2)
    ones = torch.ones_like(d_o)
    gi = ops.sdpa_bwd(q, k, vt, o, ones, lse, N).float().reshape(B, N, 3, h, 64)
    colsum = gi[:, :, 2].sum(dim=1)                                   # [B, h, 64]
    assert (colsum - N).abs().max().item() < 0.02 * N, (colsum.min().item(), colsum.max().item())
    # <q, dq> = <k, dk> per (image, head): both equal scale * sum_ij dS_ij S_ij (random dO run)
    gq = g1.float().reshape(B, N, 3, h, 64)
    qr = ops.q_from_fragment_major(q)[:, :, :N].float() / ops.QSCALE  # [B, h, N, 64]; the workspace holds q * QSCALE
    kr = k[:, :, :N].float()
    lhs = (qr * gq[:, :, 0].permute(0, 2, 1, 3)).sum(dim=(2, 3))
    rhs = (kr * gq[:, :, 1].permute(0, 2, 1, 3)).sum(dim=(2, 3))
    scale = torch.maximum(lhs.abs(), rhs.abs()).max().item() + 1e-6
    assert ((lhs - rhs).abs().max().item() / scale) < 3e-2, (lhs, rhs)


@pytest.mark.parametrize("B,N,h", [(2, 4197, 12), (1, 6501, 16), (2, 197, 3), (1, 64, 2), (3, 65, 1)])
def test_sdpa_bwd_transposing_reads_equal_the_transposed_copy_kernels(ops, B, N, h):
    """as_sdpa_bwd's two bf16 routes against each other: round 4's kernels (one row-major tile image per operand, column
    fragments through ds_read_b64_tr_b16, row statistics as MFMA C operands) and round 3's (q^T / k^T / dO^T copies;
    AS_BWD_TR=0, read once per process: a child process).  Same tiles, same order of the sums; the only arithmetic
    difference is where -lse2 / -delta enter (C operand instead of a subtraction after the MFMA), so a P or dS may round to
    the neighbouring bf16: 5e-3 of each gradient's range (measured 2.6e-3 / 3.3e-3 at the ViT-B / ViT-L sizes).  NaN in
    the padded rows of the workspaces must not leak on either route."""
    import subprocess, sys, os
    g = torch.Generator().manual_seed(5 * N + h)
    x, wqkv, bqkv, _, _ = _attn_inputs(B, N, h, 5 * N + h, scale=2.0)
    d_o = torch.randn(B, N, 64 * h, generator=g)
    path = "/tmp/as_bwd_route_%d_%d_%d.pt" % (B, N, h)
    torch.save((x, wqkv, bqkv, d_o), path + ".in")
    code = """
import sys, torch
sys.path.insert(0, {root!r})
from attentionshift_amd import ops
x, wqkv, bqkv, d_o = torch.load({inp!r})
q, k, vt = ops.qkv_fwd(x.bfloat16().cuda(), wqkv.bfloat16().cuda(), bqkv.cuda(), {h})
k[:, :, {N}:] = float('nan'); vt[:, :, :, {N}:] = float('nan')
o, lse = ops.sdpa_fwd(q, k, vt, {N})
out = ops.sdpa_bwd(q, k, vt, o, d_o.bfloat16().cuda(), lse, {N})
torch.save(out.cpu(), {outp!r})
""".format(root=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), inp=path + ".in", h=h, N=N, outp=path)
    outs = []
    for env in ({"AS_BWD_TR": "0"}, {}):
        cp = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
        assert cp.returncode == 0, cp.stderr[-2000:]
        outs.append(torch.load(path).float())
    old, new = outs
    assert torch.isfinite(old).all() and torch.isfinite(new).all()
    o3, n3 = old.reshape(B, N, 3, h * 64), new.reshape(B, N, 3, h * 64)
    for i, name in enumerate(("dq", "dk", "dv")):
        rng = float(o3[:, :, i].abs().max())
        assert float((o3[:, :, i] - n3[:, :, i]).abs().max()) <= 5e-3 * rng, (name, float((o3[:, :, i] - n3[:, :, i]).abs().max()) / rng)


@pytest.mark.parametrize("B,N,h", [(2, 297, 3), (1, 130, 2)])
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-4), (torch.bfloat16, 4e-2)])
def test_attention_module_bwd_matches_autograd(ops, dtype, tol, B, N, h):
    """as_attn_bwd through the torch.autograd bridge (attentionshift_amd.autograd.AttentionFn) vs autograd of the
    oracle's Attention.forward (fp64) on the same rounded operands: dx, dWqkv, dbqkv, dWproj, dbproj."""
    from attentionshift_amd import autograd as AG
    x, wqkv, bqkv, wproj, bproj = _attn_inputs(B, N, h, 91, scale=2.0)
    g = torch.Generator().manual_seed(5)
    dout = torch.randn(B, N, 64 * h, generator=g)
    xd, wq, wp, dod = x.to(dtype), wqkv.to(dtype), wproj.to(dtype), dout.to(dtype)
    with torch.enable_grad():
        ref_in = [t.double().requires_grad_(True) for t in (xd, wq, bqkv, wp, bproj)]
        out_ref, _ = O.attention(ref_in[0], ref_in[1], ref_in[2], ref_in[3], ref_in[4], h)
        out_ref.backward(dod.double())
        got_in = [dev(t).requires_grad_(True) for t in (xd, wq, bqkv, wp, bproj)]
        out = AG.attention(got_in[0], got_in[1], got_in[2], got_in[3], got_in[4], h)
        out.backward(dev(dod))
    mx, _ = rel_to_range(out_ref.detach().float(), out.detach().float())
    assert mx < tol, ("out", mx)
    for name, r, gt in zip(("dx", "dWqkv", "dbqkv", "dWproj", "dbproj"), ref_in, got_in):
        assert gt.grad is not None, name
        mx, mean = rel_to_range(r.grad.float(), gt.grad.float())
        assert mx < tol, (name, mx, mean)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-3), (torch.bfloat16, 3e-2)])
def test_rollout_rows_match_oracle(ops, dtype, tol):
    """A3: row-sliced roll-out from recomputed attention tiles vs attns_project_to_feature rows."""
    B, N, h, T, Lc = 2, 297, 3, 100, 4
    states, attns = [], []
    for l in range(Lc):
        x, wqkv, bqkv, wproj, bproj = _attn_inputs(B, N, h, 40 + l, scale=3.0)
        xd, wq, wp = x.to(dtype), wqkv.to(dtype), wproj.to(dtype)
        _, p = O.attention(xd.float(), wq.float(), bqkv, wp.float(), bproj, h)
        attns.append(p.mean(1))
        _, st = ops.attention_fwd(dev(xd), dev(wq), dev(bqkv), dev(wp), dev(bproj), h)
        states.append(st)
    ref = O.rollout_rows(attns, T)
    got = ops.rollout_rows(states, T)
    mx, _ = rel_to_range(ref, got)
    assert mx < tol, mx


# ------------------------------------------------------------------------------------------------
# Part B
# ------------------------------------------------------------------------------------------------
def _blobs(seed, M, H, W, p=0.55):
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(M, 1, max(H // 8, 1), max(W // 8, 1), generator=g)
    img = torch.nn.functional.interpolate(low, (H, W), mode="bilinear")[:, 0]
    return (img > p).to(torch.uint8)


@pytest.mark.parametrize("M,H,W", [(3, 64, 64), (2, 224, 224), (1, 37, 53), (2, 1024, 1024)])
def test_ccl_bit_exact(ops, M, H, W):
    img = _blobs(H + W, M, H, W)
    img[0, 0, 0] = 1
    img[-1, -1, -1] = 1
    ref = O.ccl_labels(img.numpy())
    got = ops.ccl_2d(dev(img))
    assert_equal(ref, got, f"ccl {M}x{H}x{W}")


def test_ccl_edge_cases(ops):
    for img in (torch.zeros(1, 16, 16, dtype=torch.uint8), torch.ones(1, 16, 16, dtype=torch.uint8),
                torch.eye(32, dtype=torch.uint8)[None],                       # diagonal: 8-connectivity
                torch.eye(32, dtype=torch.uint8).flip(1)[None],               # anti-diagonal (NE links)
                (torch.arange(40 * 40).reshape(1, 40, 40) % 2).to(torch.uint8)):  # vertical stripes
        assert_equal(O.ccl_labels(img.numpy()), ops.ccl_2d(dev(img)), "ccl edge case")
    # serpentine: a single component whose min index is far from most pixels
    s = torch.zeros(1, 33, 33, dtype=torch.uint8)
    s[0, ::2, :] = 1
    s[0, 1::4, -1] = 1
    s[0, 3::4, 0] = 1
    assert_equal(O.ccl_labels(s.numpy()), ops.ccl_2d(dev(s)), "ccl serpentine")


@pytest.mark.parametrize("tag", ["tiny224", "mid320"])
def test_cam_boxes_match_golden(ops, golden, tag):
    g = golden(f"shift_{tag}")
    inp = shift_case_inputs(g)
    Lc, G, hp, wp = inp["cams"].shape
    cams = inp["cams"].reshape(Lc * G, hp, wp)
    pts = inp["points"].repeat(Lc, 1)
    boxes, status, up, mm = ops.cam_boxes(dev(cams), dev(pts), float(g["cam_thr"]), float(g["area_ratio"]), 16, True)
    assert_equal(torch.stack((up.flatten(1).min(1)[0], up.flatten(1).max(1)[0]), dim=1), mm, "per-map min/max")
    assert_equal(O.upsample_bilinear(inp["cams"], hp * 16, wp * 16).reshape(Lc * G, hp * 16, wp * 16), up, "upsampled CAMs")
    got = boxes.reshape(Lc, G, 4).permute(1, 0, 2)
    assert_equal(t(g["ref_boxes"]), got, "CAM boxes vs reference")
    assert_equal(t(g["ref_kept_area"]).int(), status.reshape(Lc, G).t().cpu(), "kept-pixel counts")


def _boxes_from_pixel_ccl(ops, up, mm, thr, ratio, pts):
    nmap = (up - mm[:, 0, None, None]) / (mm[:, 1, None, None] - mm[:, 0, None, None]).clamp_min(1e-6)
    labels = ops.ccl_2d((nmap >= thr).to(torch.uint8).contiguous()).cpu()
    H, W = up.shape[-2:]
    out = []
    for m in range(up.shape[0]):
        lab = labels[m]
        ids, areas = torch.unique(lab[lab > 0], return_counts=True)
        kept = torch.isin(lab, ids[areas.float() >= ratio * areas.max().float()])
        ys, xs = kept.nonzero(as_tuple=True)
        xmin, xmax, ymin, ymax = float(xs.min()), float(xs.max()), float(ys.min()), float(ys.max())
        xc, yc = float(pts[m, 0]), float(pts[m, 1])
        bx = (xmin, min(2 * xc - xmin, float(W))) if abs(xc - xmin) > abs(xc - xmax) else (max(2 * xc - xmax, 0.0), xmax)
        by = (ymin, min(2 * yc - ymin, float(H))) if abs(yc - ymin) > abs(yc - ymax) else (max(2 * yc - ymax, 0.0), ymax)
        out.append((int(kept.sum()), [bx[0], by[0], bx[1], by[1]]))
    return out


def test_cam_boxes_wide_maps_match_pixel_ccl(ops):
    """1280-pixel-wide maps (ViT-L, BASELINE config 4): rows span more 64-column words than the run kernel keeps in
    registers, so runs are carried across its column trips; foreground touching the right border included."""
    gen = torch.Generator().manual_seed(19)
    M, hp, wp = 4, 80, 80
    cams = 0.3 * torch.rand(M, hp, wp, generator=gen)
    cams[0, 10:60, 5:78] += 1.0                               # crosses the 1024-column trip boundary
    cams[1, 20:40, 60:80] += 1.0                              # touches the right border
    cams[2, 5:15, 2:30] += 1.0
    cams[2, 40:70, 50:79] += 0.9                              # two blobs, one filtered by area
    cams[3, :, :] += torch.linspace(0, 1, wp)[None, :]         # a ramp: one run per row ending at the border
    pts = torch.tensor([[600., 500.]] * M)
    boxes, status, up, mm = ops.cam_boxes(dev(cams), dev(pts), 0.5, 0.5, 16, True)
    for m, (area, box) in enumerate(_boxes_from_pixel_ccl(ops, up, mm, 0.5, 0.5, pts)):
        assert int(status[m]) == area, m
        assert boxes[m].tolist() == box, m


def test_cam_boxes_more_runs_than_fit_lds_match_pixel_ccl(ops):
    """A 64x64 checkerboard upsampled to 1024^2 has ~32 runs in every row (> 18432 per map): the component stage then
    works on its workspace arrays instead of LDS.  Same partition as the per-pixel labelling."""
    yy, xx = torch.meshgrid(torch.arange(64), torch.arange(64), indexing="ij")
    board = ((yy + xx) % 2).float()
    cams = torch.stack((board, 1 - board))
    cams[0, 20:30, 20:30] = 1.0                               # one block larger than the rest
    cams[1, 5:9, 40:50] = 1.0
    pts = torch.tensor([[400., 400.], [700., 100.]])
    boxes, status, up, mm = ops.cam_boxes(dev(cams), dev(pts), 0.6, 0.5, 16, True)
    for m, (area, box) in enumerate(_boxes_from_pixel_ccl(ops, up, mm, 0.6, 0.5, pts)):
        assert int(status[m]) == area, m
        assert boxes[m].tolist() == box, m


def test_cam_boxes_noise_maps_match_pixel_ccl(ops):
    """Speckled maps (hundreds of components, dozens of runs per row): the run-based box stage must give what the
    per-pixel labelling (as_ccl_2d, itself pinned to scipy) gives -- kept area and tight box per map."""
    gen = torch.Generator().manual_seed(11)
    M, hp, wp = 6, 20, 24
    cams = torch.rand(M, hp, wp, generator=gen)
    cams[0, 5:12, 6:15] += 1.0                               # one dominant blob, the rest pure noise
    pts = torch.full((M, 2), 100.0)
    boxes, status, up, mm = ops.cam_boxes(dev(cams), dev(pts), 0.45, 0.5, 16, True)
    nmap = (up - mm[:, 0, None, None]) / (mm[:, 1, None, None] - mm[:, 0, None, None]).clamp_min(1e-6)
    fg = (nmap >= 0.45).to(torch.uint8)
    labels = ops.ccl_2d(fg.contiguous()).cpu()
    H, W = hp * 16, wp * 16
    for m in range(M):
        lab = labels[m]
        ids, areas = torch.unique(lab[lab > 0], return_counts=True)
        keep = ids[areas.float() >= 0.5 * areas.max().float()]
        kept = torch.isin(lab, keep)
        assert int(status[m]) == int(kept.sum()), m
        ys, xs = kept.nonzero(as_tuple=True)
        xmin, xmax, ymin, ymax = float(xs.min()), float(xs.max()), float(ys.min()), float(ys.max())
        xc = yc = 100.0                                      # 'expand' about the point (stdroi:97-115)
        if abs(xc - xmin) > abs(xc - xmax):
            want_x = (xmin, min(2 * xc - xmin, float(W)))
        else:
            want_x = (max(2 * xc - xmax, 0.0), xmax)
        if abs(yc - ymin) > abs(yc - ymax):
            want_y = (ymin, min(2 * yc - ymin, float(H)))
        else:
            want_y = (max(2 * yc - ymax, 0.0), ymax)
        assert boxes[m].tolist() == [want_x[0], want_y[0], want_x[1], want_y[1]], m


@pytest.mark.parametrize("G,hp,wp", [(3, 14, 14), (1, 8, 12), (5, 20, 16), (11, 9, 72)])
def test_cam_sample_masks_bit_exact(ops, G, hp, wp):
    """as_cam_sample_masks == thresholding the materialised normalised maps (norm_attns on the upsampled CAMs)."""
    gen = torch.Generator().manual_seed(5 + G)
    M = 3 * G
    cams = torch.rand(M, hp, wp, generator=gen)
    pts = torch.full((M, 2), 20.0)
    _, _, up, mm = ops.cam_boxes(dev(cams), dev(pts), 0.2, 0.5, 16, True)
    idx = torch.randperm(M, generator=gen)[:G].to(torch.int32)
    masks, counts = ops.cam_sample_masks(dev(cams), dev(idx), mm, 0.1, 0.2, 16)
    sel = idx.long().to(up.device)
    nm = (up[sel] - mm[sel, 0, None, None]) / (mm[sel, 1, None, None] - mm[sel, 0, None, None])
    tot = nm[0].clone()                                   # sequential sum over the maps, then one division
    for g_ in range(1, G):
        tot = tot + nm[g_]
    want = torch.cat((nm < 0.1, nm >= 0.2, ((tot / G) < 0.1)[None])).to(torch.uint8)
    assert_equal(want, masks, "candidate masks")
    assert_equal(want.flatten(1).sum(1).int(), counts, "candidate counts")


@pytest.mark.parametrize("k", [21, 1])
def test_mask_candidates_equal_the_three_separate_calls(ops, k):
    """as_mask_candidates == crop_threshold_erode(fg, crops, k) / (bg, crops, 1) / (fg, whole image, 1), bitwise."""
    gen = torch.Generator().manual_seed(23)
    G, H, W = 3, 160, 224
    low = torch.rand(2, G, H // 16, W // 16, generator=gen)
    fg, bg = (torch.nn.functional.interpolate(low[i][None], scale_factor=16, mode="bilinear")[0].contiguous() for i in range(2))
    crops = torch.tensor([[10, 5, 150, 140], [0, 0, W, H], [200, 100, 190, 120]], dtype=torch.int32)   # last: empty crop
    pos, neg, pseudo, counts = ops.mask_candidates(dev(fg), dev(bg), dev(crops), 0.35, 0.8, 0.5, k)
    p0, c0 = ops.crop_threshold_erode(dev(fg), dev(crops), 0.35, True, k)
    p1, c1 = ops.crop_threshold_erode(dev(bg), dev(crops), 0.8, True, 1)
    p2, c2 = ops.crop_threshold_erode(dev(fg), None, 0.5, True, 1)
    assert_equal(p0, pos, "pos candidates"); assert_equal(p1, neg, "neg candidates"); assert_equal(p2, pseudo, "pseudo mask")
    assert_equal(torch.stack((c0, c1, c2)), counts, "counts")
    assert int(counts[0, 0]) > 0 and int(counts[1, 1]) > 0 and int(counts[0, 2]) == 0


def test_filter_parts_and_part_stats_equal_the_torch_forms(ops):
    """as_filter_parts / as_part_stats vs the tensor-op restatements of stdroi:263-271 and :222-262 (exact: integer /
    quarter-valued sums)."""
    from attentionshift_amd import roi_head as RH
    gen = torch.Generator().manual_seed(31)
    G, P, hp, wp = 3, 20, 20, 24
    sim = torch.rand(G, P, hp, wp, generator=gen)
    sim[:, ::3] = sim[:, ::3] * 0.5 + 0.5
    fg = (torch.randint(0, 5, (G, hp, wp), generator=gen).float() / 4)
    assert_equal(RH.filter_parts(sim, fg, 0.85), ops.filter_parts(dev(sim), dev(fg)), "keep")
    maps = sim.flatten(0, 1)
    maps[5] = 0.3                                              # a constant map: every pixel is at the peak
    owner = torch.arange(G).repeat_interleave(P)
    rois = torch.tensor([[0., 0., 200., 200.], [100., 50., 384., 320.], [0., 0., 10., 10.]])
    c, yx, area, inside = ops.part_stats(dev(maps), dev(rois), dev(owner), 16)
    peak = maps.flatten(1).max(1)[0][:, None, None]
    at = (maps >= peak).float()
    cnt = at.sum(dim=[-2, -1])
    cy = (at * torch.arange(hp).float()[None, :, None]).sum(dim=[-2, -1]) / cnt
    cx = (at * torch.arange(wp).float()[None, None, :]).sum(dim=[-2, -1]) / cnt
    want_c = (torch.stack((cx, cy), dim=1) + 0.5) * 16
    box = rois[owner]
    assert_equal(want_c, c, "centres"); assert_equal(torch.stack((cy.long(), cx.long()), 1), yx, "integer centroids")
    assert_equal((maps > 0.9).sum(dim=[-2, -1]), area, "areas")
    assert_equal((want_c[:, 0] >= box[:, 0]) & (want_c[:, 0] <= box[:, 2]) & (want_c[:, 1] >= box[:, 1]) & (want_c[:, 1] <= box[:, 3]),
                 inside, "inside")


@pytest.mark.parametrize("G,hp,wp,thr", [(3, 14, 14, 0.35), (2, 9, 20, 0.5), (5, 6, 6, 0.35)])
def test_semantic_prestage_matches_oracle(ops, G, hp, wp, thr):
    """erode_11(map > thr) -> bilinear /16 -> binarise (stdroi:2011-2020) in one launch vs max-pool + interpolate."""
    gen = torch.Generator().manual_seed(17 + G)
    low = torch.rand(G, hp, wp, generator=gen)
    m = torch.nn.functional.interpolate(low[None], scale_factor=16, mode="bilinear")[0]      # blobs with soft edges
    m[:, :3] = 1.0                                            # foreground touching the image border (padding rule)
    fg_inter, _bg, fg_bin = O.semantic_prestage(m, m, (hp, wp), thr)
    got_inter, got_mask, got_cnt = ops.semantic_prestage(dev(m), thr, 11, 16)
    assert_equal(fg_inter, got_inter, "fg_inter")
    assert_equal(fg_bin.to(torch.uint8), got_mask, "binary patch map")
    assert_equal(fg_bin.flatten(1).sum(1).int(), got_cnt, "counts")


def _shift_inputs_dev(g, inp):
    hp, wp, G = int(g["hp"]), int(g["wp"]), int(g["G"])
    rois = t(g["rois"])
    fg_inter, bg_inter, fg_bin = O.semantic_prestage(t(g["map_fg_last"]), t(g["map_bg_last"]), (hp, wp), float(g["pos_thr"]))
    seeds = O.grid_seed_coords(fg_bin, rois)
    feat_tok = inp["vit_feat"].flatten(1).t().contiguous()            # [Np, C]
    prot = inp["vit_feat"].permute(1, 2, 0)[seeds[..., 0], seeds[..., 1]].contiguous()
    box_patch = (rois // 16).int()
    return feat_tok, prot, box_patch


@pytest.mark.parametrize("tag", ["tiny224", "mid320"])
def test_cosine_shift_matches_golden(ops, golden, tag):
    """B4 vs the reference's cosine_shift_batch: prototypes/sim 1e-3 relative, cluster assignment
    (argmax) bit-exact at every iteration, tau to the 1-cos noise floor."""
    g = golden(f"shift_{tag}")
    inp = shift_case_inputs(g)
    hp, wp, G, S = int(g["hp"]), int(g["wp"]), int(g["G"]), int(g["n_shift"])
    feat_tok, prot, box_patch = _shift_inputs_dev(g, inp)
    obj_img = torch.zeros(G, dtype=torch.int32)
    pout, sim, assign, tau = ops.cosine_shift(dev(feat_tok[None]), dev(box_patch), dev(obj_img), dev(prot), S, hp, wp,
                                              return_trace=True)
    assert_equal(t(g["ref_assign"]), assign, "cluster assignment (all iterations)")
    assert_close(t(g["ref_tau"]), tau, 1e-3, 2e-6, "tau")
    assert_close(t(g["ref_prot"]), pout.reshape(-1, pout.shape[-1]), 1e-3, 1e-4, "prototypes")
    assert_close(t(g["ref_sim"]).flatten(1), sim.reshape(-1, hp * wp).clamp(min=0), 1e-3, 1e-5, "sim")


def test_cosine_shift_ties_and_batch(ops):
    """Duplicate seeds -> lowest index wins; two images in one call == two separate calls."""
    gen = torch.Generator().manual_seed(11)
    hp = wp = 12
    C, P = 64, 20
    feat = torch.randn(2, hp * wp, C, generator=gen)
    boxes = torch.tensor([[1, 1, 8, 9], [0, 0, 11, 11], [3, 2, 10, 6]], dtype=torch.int32)
    obj_img = torch.tensor([0, 1, 1], dtype=torch.int32)
    prot = torch.randn(3, P, C, generator=gen)
    prot[0, 5] = prot[0, 2]
    prot[0, 9] = prot[0, 2]
    pout, sim, assign, tau = ops.cosine_shift(dev(feat), dev(boxes), dev(obj_img), dev(prot), 3, hp, wp, return_trace=True)
    a0 = assign[0, 0].cpu()
    assert not ((a0 == 5) | (a0 == 9)).any(), "duplicates must lose the tie to prototype 2"
    for gi in range(3):
        b = int(obj_img[gi])
        p1, s1, a1, t1 = ops.cosine_shift(dev(feat[b:b + 1]), dev(boxes[gi:gi + 1]), dev(torch.zeros(1, dtype=torch.int32)),
                                          dev(prot[gi:gi + 1]), 3, hp, wp, return_trace=True)
        assert_equal(a1[:, 0], assign[:, gi], "batched == single (assign)")
        assert_equal(p1[0], pout[gi], "batched == single (prototypes, bitwise)")
        assert_equal(s1[0], sim[gi], "batched == single (sim, bitwise)")
    # oracle on the same inputs
    trace = []
    for gi in range(3):
        b = int(obj_img[gi])
        inbox = O.box_mask(boxes[gi:gi + 1].float(), (hp, wp)).flatten(1)
        tr = []
        po, so = O.cosine_shift(prot[gi:gi + 1].clone(), feat[b][None] * inbox[..., None], feat[b], n_shift=3, trace=tr)
        assert_equal(torch.stack([x[0][0] for x in tr]).int(), assign[:, gi], f"assign vs oracle obj {gi}")
        assert_close(po, pout[gi], 1e-3, 1e-4, "prot vs oracle")
        assert_close(so, sim[gi], 1e-3, 1e-5, "sim vs oracle")


def test_cosine_shift_reads_the_callers_view_of_last_feat_in_place(ops):
    """as_cosine_shift_strided: vit_feat as the reference's caller builds it -- a view of last_feat [B, 1 + Np, C] without the
    cls row (two_stage_point_align.py:77), images (1 + Np) * C floats apart -- gives bitwise the result of the contiguous copy."""
    from attentionshift_amd import synthetic
    hp, wp, C, B = 14, 18, 192, 3
    feats, boxes, prots, obj = [], [], [], []
    for b in range(B):
        inp = synthetic.shift_inputs(300 + b, hp, wp, C, 2, 1)
        f = inp["vit_feat"].flatten(1).t().contiguous()
        feats.append(f)
        pb = inp["patch_boxes"].int()
        boxes.append(pb)
        for gi in range(2):
            x0, y0, x1, y1 = pb[gi].tolist()
            idx = (torch.linspace(y0, y1, 5).long()[:, None] * wp + torch.linspace(x0, x1, 4).long()[None, :]).flatten()
            prots.append(f[idx])
            obj.append(b)
    last = torch.randn(B, 1 + hp * wp, C)
    last[:, 1:] = torch.stack(feats)
    last = last.cuda()
    view = last[:, 1:]                                             # [B, Np, C], stride(0) = (1 + Np) * C
    assert not view.is_contiguous()
    args = (dev(torch.cat(boxes)), dev(torch.tensor(obj, dtype=torch.int32)), dev(torch.stack(prots)), 4, hp, wp)
    r_view = ops.cosine_shift(view, *args, return_trace=True)
    r_copy = ops.cosine_shift(view.contiguous(), *args, return_trace=True)
    for a, b_ in zip(r_view, r_copy):
        assert_equal(b_, a, "strided view vs contiguous copy")
    with pytest.raises(Exception):
        ops.cosine_shift(last.transpose(1, 2)[:, :, 1:].transpose(1, 2)[:, :, ::2], *args)      # rows not contiguous


def test_cosine_shift_full_size_properties(ops):
    """BASELINE config-2 shape (B=2, 64x64 patches, C=768, G=3/img, P=20, S=5): size-independent
    properties -- cosine range, assignment range, determinism (two runs bitwise equal), and that the
    final sim equals a direct cosine of the returned prototypes."""
    from attentionshift_amd import synthetic
    hp = wp = 64
    feats, boxes, prots, obj = [], [], [], []
    for b in range(2):
        inp = synthetic.shift_inputs(100 + b, hp, wp, 768, 3, 1)
        f = inp["vit_feat"].flatten(1).t().contiguous()
        feats.append(f)
        pb = inp["patch_boxes"].int()
        boxes.append(pb)
        for gi in range(3):
            x0, y0, x1, y1 = pb[gi].tolist()
            ys = torch.linspace(y0, y1, 5).long()
            xs = torch.linspace(x0, x1, 4).long()
            idx = (ys[:, None] * wp + xs[None, :]).flatten()
            prots.append(f[idx])
            obj.append(b)
    feat = torch.stack(feats)
    box_patch = torch.cat(boxes)
    prot = torch.stack(prots)
    obj_img = torch.tensor(obj, dtype=torch.int32)
    r1 = ops.cosine_shift(dev(feat), dev(box_patch), dev(obj_img), dev(prot), 5, hp, wp, return_trace=True)
    r2 = ops.cosine_shift(dev(feat), dev(box_patch), dev(obj_img), dev(prot), 5, hp, wp, return_trace=True)
    for a, b in zip(r1, r2):
        assert_equal(a, b, "determinism")
    pout, sim, assign, tau = r1
    assert sim.abs().max().item() <= 1.0 + 1e-5
    assert int(assign.min()) >= 0 and int(assign.max()) < 20
    assert torch.isfinite(pout).all() and torch.isfinite(tau).all() and (tau >= 1e-10).all()
    direct = O.cos_matrix(pout.cpu(), feat[obj_img.long()])
    assert_close(direct, sim, 1e-3, 1e-5, "final sim == cos(prot, feat)")


@pytest.mark.parametrize("tag", ["tiny224", "mid320"])
def test_refine_and_instance_maps_match_golden(ops, golden, tag):
    """B2 vs get_cosine_similarity_refined_map (given the same sampled points): maps 1e-3."""
    g = golden(f"shift_{tag}")
    inp = shift_case_inputs(g)
    hp, wp, G = int(g["hp"]), int(g["wp"]), int(g["G"])
    feat = inp["vit_feat"]
    feat_tok = feat.flatten(1).t().contiguous()
    rois = t(g["rois"])
    box_patch = (rois // 16).int()
    seeds_fg = O.seed_features(t(g["points_fg"]), feat)
    seeds_bg = O.seed_features(t(g["points_bg"]), feat)
    sim_fg, f_fg = ops.refine_similarity(dev(feat_tok), dev(seeds_fg), dev(box_patch), G, 2, float(g["obj_tau"]), True, hp, wp)
    sim_bg, f_bg = ops.refine_similarity(dev(feat_tok), dev(seeds_bg), dev(box_patch), G, 2, float(g["obj_tau"]), False, hp, wp)
    o_fg, _ = O.refined_similarity(t(g["points_fg"]), feat, rois, 2, float(g["obj_tau"]), True)
    o_bg, _ = O.refined_similarity(t(g["points_bg"]), feat, rois, 2, float(g["obj_tau"]), False)
    assert_close(o_fg.flatten(2), sim_fg, 1e-3, 1e-5, "patch-grid fg maps vs oracle")
    assert_close(o_bg.flatten(2), sim_bg, 1e-3, 1e-5, "patch-grid bg maps vs oracle")
    assert_close(t(g["fg_feat"]), f_fg, 1e-3, 1e-4, "refined fg seeds vs reference")
    assert_close(t(g["bg_feat"]), f_bg, 1e-3, 1e-4, "refined bg seeds vs reference")
    map_fg, map_bg = ops.instance_maps(sim_fg, sim_bg, G, hp, wp)
    assert_close(t(g["map_fg_last"]), map_fg[-1], 1e-3, 1e-5, "map_fg[-1] vs reference")
    assert_close(t(g["map_bg_last"]), map_bg[-1], 1e-3, 1e-5, "map_bg[-1] vs reference")
    assert_close(t(g["map_fg_sub"]), map_fg[:, :, ::4, ::4], 1e-3, 1e-5, "map_fg levels vs reference")
    assert_close(t(g["map_bg_sub"]), map_bg[:, :, ::4, ::4], 1e-3, 1e-5, "map_bg levels vs reference")
    # the elementwise tail is bit-exact given identical patch-grid maps
    m_fg, m_bg = ops.instance_maps(dev(o_fg.flatten(2)), dev(o_bg.flatten(2)), G, hp, wp)
    H, W = hp * 16, wp * 16
    up_fg = O.upsample_bilinear(o_fg, H, W)[:, :G]
    up_bg = O.upsample_bilinear(o_bg, H, W)
    ret = (1 - up_bg) * up_fg
    assert_equal(ret / ret.flatten(-2).max(-1)[0][..., None, None].clamp(1e-8), m_fg, "instance map arithmetic (bitwise)")


def test_crop_threshold_erode_matches_torch(ops):
    """B2'/B3 candidate masks vs erode((crop > cropmax*thr)) built from torch max_pool2d (stdroi:442, :2011)."""
    g = torch.Generator().manual_seed(12)
    M, H, W = 4, 160, 200
    low = torch.rand(M, 1, 10, 13, generator=g)
    maps = torch.nn.functional.interpolate(low, (H, W), mode="bilinear")[:, 0].contiguous()
    crops = torch.tensor([[10, 20, 150, 120], [0, 0, 200, 160], [50, 60, 51, 61], [190, 150, 260, 300]], dtype=torch.int32)
    for rel, thr, k in ((True, 0.6, 21), (True, 0.8, 1), (False, 0.5, 11)):
        for use_crops in (True, False):
            mask, cnt = ops.crop_threshold_erode(dev(maps), dev(crops) if use_crops else None, thr, rel, k)
            ref = torch.zeros(M, H, W, dtype=torch.uint8)
            for m in range(M):
                x0, y0, x1, y1 = crops[m].tolist() if use_crops else (0, 0, W, H)
                sub = maps[m][y0:y1, x0:x1]
                if sub.numel() == 0:
                    continue
                b = (sub > (sub.max() * thr if rel else thr)).float()
                if k > 1:
                    b = O.erode(b, k)
                ref[m][y0:y1, x0:x1] = b.to(torch.uint8)
            assert_equal(ref, mask, f"mask rel={rel} k={k} crops={use_crops}")
            assert_equal(ref.flatten(1).sum(1).int(), cnt, "counts")


def test_rank_select_matches_nonzero(ops):
    g = torch.Generator().manual_seed(13)
    for M, HW, dens in ((3, 1024 * 1024, 0.3), (2, 4096 * 3 + 48, 0.01), (1, 160, 0.5), (2, 50176, 0.9)):
        mask = (torch.rand(M, HW, generator=g) < dens).to(torch.uint8)
        mask[0, :5] = 1
        mask[-1, -3:] = 1
        cnt = mask.sum(1)
        ranks = torch.stack([torch.randint(int(cnt[m]), (20,), generator=g) for m in range(M)])
        ranks[:, 0] = 0
        ranks[:, 1] = cnt - 1
        ref = torch.stack([mask[m].nonzero()[:, 0][ranks[m]] for m in range(M)])
        got = ops.rank_select(dev(mask), dev(ranks))
        assert_equal(ref, got, f"rank select M={M} HW={HW}")
        beyond = ops.rank_select(dev(mask), dev(cnt[:, None] + torch.zeros(M, 1, dtype=torch.long)))
        assert (beyond.cpu() == -1).all()


def test_merge_parts_equals_the_tensor_op_chain(ops):
    """as_merge_parts (links, greedy grouping, merged prototypes in one launch) against normalise / matmul / >= thr /
    as_merge_plan / matmul(weight, prot) / (sum + 1e-8) (stdroi:278-294; oracle.merge_parts), incl. the slot cap flag."""
    g = torch.Generator().manual_seed(31)
    for G, P, C, slots in ((3, 20, 768, 20), (7, 20, 1024, 8), (2, 5, 64, 5), (4, 32, 192, 3)):
        base = torch.randn(G, 4, C, generator=g)
        prot = base[:, torch.randint(4, (P,), generator=g)] + 0.25 * torch.randn(G, P, C, generator=g)   # a few tight clusters
        prot[0, 1] = prot[0, 0]                                # an exact duplicate (cos = 1)
        keep = torch.rand(G, P, generator=g) < 0.7
        keep[-1] = False                                       # an object that keeps nothing
        u = prot / prot.norm(dim=-1, keepdim=True).clamp_min(1e-8)
        link = (u @ u.transpose(1, 2)) >= 0.85
        groups, ngroups = ops.merge_plan(dev(keep), dev(link))
        groups, ngroups = groups.cpu(), ngroups.cpu()
        wgt = ((groups[:, :slots, None] >> torch.arange(P, dtype=torch.int32)) & 1).float()
        ref = torch.bmm(wgt, prot) / (wgt.sum(-1, keepdim=True) + 1e-8)
        flag = torch.zeros(1, dtype=torch.int32).cuda()
        merged, ng = ops.merge_parts(dev(prot), dev(keep), 0.85, slots, flag)
        assert_equal(ngroups.clamp(max=slots), ng, f"group counts G={G} P={P}")
        assert bool(flag.item()) == bool((ngroups > slots).any()), "slot-cap flag"
        assert_close(ref, merged, 1e-6, 1e-6, f"merged prototypes G={G} P={P} C={C}")
        ref_o = [O.merge_parts([prot[i][keep[i]]], 0.85)[0] if keep[i].any() else [] for i in range(G)] if hasattr(O, "merge_parts") else None
        if ref_o is not None and slots == P:
            for i in range(G):
                n = int(ng[i])
                assert n == (0 if isinstance(ref_o[i], list) else ref_o[i].shape[0]), f"object {i}: groups vs oracle"
                if n:
                    assert_close(ref_o[i], merged[i, :n], 1e-5, 1e-6, f"object {i}: merged prototypes vs oracle")


def test_assemble_tokens_equals_the_add_and_slice_writes(ops):
    """as_assemble_tokens against prepare_tokens' tensor ops (visual_transformer_det.py:192-214): bit for bit, bf16 and fp32
    projections, several token counts."""
    g = torch.Generator().manual_seed(47)
    for B, Np, T, D, dt in ((2, 4096, 100, 768, torch.bfloat16), (1, 196, 5, 64, torch.float32), (3, 49, 1, 192, torch.bfloat16)):
        emb = torch.randn(B, Np, D, generator=g).to(dt)
        pos = torch.randn(1, 1 + Np, D, generator=g)
        cls, pt, ptpos = torch.randn(1, 1, D, generator=g), torch.randn(1, T, D, generator=g), torch.randn(1, T, D, generator=g)
        ref = torch.empty(B, 1 + Np + T, D)
        torch.add(emb.float(), pos[:, 1:], out=ref[:, 1:1 + Np])
        ref[:, :1] = cls + pos[:, :1]
        ref[:, 1 + Np:] = pt + ptpos
        table = torch.cat((cls + pos[:, :1], pos[:, 1:], pt + ptpos), dim=1)[0].contiguous()
        assert_equal(ref, ops.assemble_tokens(dev(emb), dev(table)), f"token tensor B={B} Np={Np} T={T} D={D} {dt}")


def test_select_median_boxes_equals_the_selector_and_its_index_chain(ops):
    """as_select_median_boxes against roi_head.median_area_selector (stable argsort of the clamped areas, the (Lc-1)//2-th
    entry) and the tensor ops it replaces around it: the chosen box, its row in the layer-major stack, `box // 16` and
    `box.int()` -- bit for bit, with ties in the areas and degenerate (negative-extent) boxes."""
    from attentionshift_amd.roi_head import median_area_selector
    g = torch.Generator().manual_seed(41)
    for counts, Lc in (((3, 3), 7), ((1, 5, 2), 4), ((7,), 7), ((2, 0, 4), 3), ((64, 33), 12)):
        per_img, rows, meta, off = [], [], [], 0
        for i, c in enumerate(counts):
            lo = torch.randint(0, 300, (Lc, c, 2), generator=g).float()
            ext = torch.randint(-20, 400, (Lc, c, 2), generator=g).float()
            b = torch.cat((lo, lo + ext), dim=-1)                               # [Lc, c, 4], some x1 < x0
            if c:
                b[Lc // 2, 0] = b[0, 0]                                        # an exact tie of two layers
            if Lc > 2 and c > 1:
                b[1, 1], b[2, 1] = torch.tensor([5., 5, 9, 3]), torch.tensor([8., 8, 2, 30])   # two zero areas (clamped)
            rows.append(b.reshape(-1, 4))
            per_img.append(b.permute(1, 0, 2).contiguous())
            meta += [[off, c, k] for k in range(c)]
            off += Lc * c
        boxes = torch.cat(rows)
        pick, chosen, map_idx, patch, ints = ops.select_median_boxes(dev(boxes), dev(torch.tensor(meta, dtype=torch.int32)), Lc, 16)
        ref_pick = torch.cat(median_area_selector(per_img))
        assert_equal(ref_pick, pick, f"median-area layer, counts {counts}")
        ref_box = torch.cat([per_img[i][torch.arange(c), p] for i, (c, p) in enumerate(zip(counts, ref_pick.split(counts)))])
        assert_equal(ref_box, chosen, "chosen boxes")
        ref_rows = torch.cat([m0 + p * c + torch.arange(c) for (c, p, m0) in
                              zip(counts, ref_pick.split(counts), [sum(Lc * x for x in counts[:i]) for i in range(len(counts))])])
        assert_equal(ref_rows.int(), map_idx, "rows of the layer-major stack")
        assert_equal((ref_box // 16).int(), patch, "patch boxes")
        assert_equal(ref_box.int(), ints, "integer crops")
        assert_equal(boxes[map_idx.long().cpu()], chosen, "map_idx addresses the chosen box")
        # another selector's choice (`pick_in`): the same indexing behind a given layer per object, out-of-range values clamped
        given = torch.randint(0, Lc, (len(meta),), generator=g)
        if len(meta) > 2:
            given[0], given[1] = Lc + 3, -2
        pick2, chosen2, rows2, patch2, ints2 = ops.select_median_boxes(dev(boxes), dev(torch.tensor(meta, dtype=torch.int32)), Lc, 16,
                                                                       pick_in=dev(given))
        want = given.clamp(0, Lc - 1)
        assert_equal(want, pick2, "given layers (clamped)")
        m = torch.tensor(meta)
        want_rows = m[:, 0] + want * m[:, 1] + m[:, 2]
        assert_equal(want_rows.int(), rows2, "rows behind the given layers")
        assert_equal(boxes[want_rows], chosen2, "boxes behind the given layers")
        assert_equal((boxes[want_rows] // 16).int(), patch2, "patch boxes behind the given layers")
        assert_equal(boxes[want_rows].int(), ints2, "integer crops behind the given layers")


def test_draw_distinct_reads_a_strided_count_table_and_ors_into_the_callers_flag(ops):
    """as_draw_distinct on the transposed view of mask_candidates' planar count rows == on its contiguous copy, and the flag
    is OR-ed into the slot the caller zeroed (neighbouring slots untouched)."""
    g = torch.Generator().manual_seed(43)
    for G in (1, 3, 7):
        planar = torch.randint(200, 5000, (3, G), generator=g).int()
        u = torch.rand(G, 32, generator=g)
        slots = torch.zeros(4, dtype=torch.int32).cuda()
        a = ops.draw_distinct(dev(planar)[:2].t(), dev(u), 10, flag=slots[3:4])
        b = ops.draw_distinct(dev(planar[:2].t()), dev(u), 10)
        for x, y, what in zip(a[:3], b[:3], ("rank_pos", "rank_neg", "is_pos")):
            assert_equal(y.cpu(), x, f"{what}, G={G}")
        assert slots.tolist() == [0, 0, 0, 0] and int(b[3]) == 0
        planar[1, 0] = 3; planar[0, 0] = 2                                   # fewer than 4 K candidates: flag
        a = ops.draw_distinct(dev(planar)[:2].t(), dev(u), 10, flag=slots[3:4])
        assert slots.tolist() == [0, 0, 0, 1]
        n_pos, n = int(planar[0, -1]), int(planar[0, -1] + planar[1, -1])
        want = []
        for v in (u[-1] * float(n)).int().clamp(max=n - 1).tolist():
            if v not in want:
                want.append(v)
        want = torch.tensor((want + [0] * 10)[:10])                           # (fewer distinct draws than asked: rank 0 fill)
        assert_equal(torch.where(want < n_pos, want, torch.zeros_like(want)).int(), a[0][-1], "positive ranks of the last object")
        assert_equal(torch.where(want < n_pos, torch.zeros_like(want), want - n_pos).int(), a[1][-1], "negative ranks")


def test_rank_draw_xy_equals_the_tensor_op_chain(ops):
    """as_rank_draw_xy (ranks derived in the selection kernel from the populations it counts) against the chain of tensor
    ops it replaces in the fast-RNG sampling paths (roi_head.sample_points_from_cams_nosync / grid_seed_nosync), bit for
    bit, incl. rows with fewer candidates than draws (flag) and empty rows (pixel 0)."""
    g = torch.Generator().manual_seed(29)
    for M, H, W, dens, K in ((7, 64, 64, 0.2, 20), (3, 128, 96, 0.6, 20), (4, 16, 16, 0.02, 20), (2, 1024, 1024, 0.3, 20)):
        mask = (torch.rand(M, H * W, generator=g) < dens).to(torch.uint8)
        if M == 4:
            mask[1] = 0                                    # an empty row
            mask[2] = 0; mask[2, 37] = 1                   # a single candidate
        counts = mask.sum(1).int()
        u = torch.rand(M, K, generator=g)
        u[0, 0] = 0.0; u[0, 1] = 0.99999994                # the ends of [0, 1)
        # mode 1: min(int(u * n), max(n - 1, 0)) -> (x, y)
        ranks = torch.minimum((u * counts.float()[:, None]).to(torch.int32), (counts[:, None] - 1).clamp(min=0))
        ref = ops.rank_select_xy(dev(mask), dev(ranks), W)
        flag = torch.zeros(1, dtype=torch.int32).cuda()
        got = ops.rank_draw_xy(dev(mask), K, W, u=dev(u), flag=flag)
        assert_equal(ref, got, f"uniform draws M={M} {H}x{W}")
        assert bool(flag.item()) == bool((counts < K).any()), "flag of the uniform draws"
        # mode 2: the k-th of K grid-strided positives -> (y, x)
        step = (counts // K).clamp(min=1)
        ranks = torch.arange(K, dtype=torch.int32)[None, :] * step[:, None].int()
        ref = ops.rank_select_xy(dev(mask), dev(ranks), W, yx=True)
        flag = torch.zeros(2, dtype=torch.int32).cuda()
        got = ops.rank_draw_xy(dev(mask), K, W, flag=flag[1:2], yx=True)
        assert_equal(ref, got, f"grid-strided seeds M={M} {H}x{W}")
        assert int(flag[0]) == 0 and bool(flag[1].item()) == bool((counts < K).any()), "flag slot of the grid seeds"
        # token ids: base + (y // div) * width + x // div, rows rotated by `rot` (the seed-feature gather index)
        if H % 16 == 0 and W % 16 == 0:
            rot, base = M // 2, 1000
            xy, pid = ops.rank_draw_xy(dev(mask), K, W, u=dev(u), patch=(None, 16, W // 16, base, rot))
            want = base + (xy[..., 1] // 16) * (W // 16) + xy[..., 0] // 16
            assert_equal(torch.roll(want.cpu(), -rot, 0), pid, f"token ids M={M} {H}x{W}")
            buf = torch.full((M + 2, K), -7, dtype=torch.int64).cuda()
            none_xy, pid2 = ops.rank_draw_xy(dev(mask), K, W, yx=True, patch=(buf[1:M + 1], 1, W, 0, 0), want_xy=False)
            assert none_xy is None and (buf[0] == -7).all() and (buf[-1] == -7).all()
            assert_equal(got[..., 0] * W + got[..., 1], buf[1:M + 1], "flat ids of the grid seeds, written into a caller's rows")


# ------------------------------------------------------------------------------------------------
# A6: Swin window attention (BASELINE config 5)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["w14_s0", "w14_s3", "w16_s3_pad", "w9_s0_pad"])
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4), (torch.bfloat16, 3e-2)])
def test_swin_block_matches_reference(ops, golden, tag, dtype, tol):
    """SwinTransformerBlock on the fused as_window_attn_fwd kernel vs the reference block's own outputs (fixture):
    shifted and unshifted windows, grids that need padding (16 -> 21, 9 -> 14)."""
    from attentionshift_amd.swin import SwinTransformerBlock
    g = golden(f"swin_{tag}")
    hw, ws, heads, C = int(g["hw"]), int(g["ws"]), int(g["heads"]), int(g["C"])
    blk = SwinTransformerBlock(C, (hw, hw), heads, window_size=ws, shift_size=int(g["shift"]), compute_dtype=dtype)
    sd = {k[2:]: t(g[k]) for k in g.files if k.startswith("p.")}
    missing = blk.load_state_dict(sd, strict=False)
    assert missing.unexpected_keys == [] and missing.missing_keys == ["attn.relative_position_index"]
    blk = blk.cuda().eval()
    y, attn = blk(dev(t(g["x"])))
    mx, _ = rel_to_range(t(g["y"]), y)
    assert mx < tol, ("block output", mx)
    mx, _ = rel_to_range(t(g["attn"]), attn)
    assert mx < tol, ("attention probabilities", mx)


@pytest.mark.parametrize("M,D,dtype,tol", [(37, 768, torch.float32, 2e-5), (1030, 768, torch.bfloat16, 2e-2),
                                            (5, 1024, torch.bfloat16, 2e-2), (300, 128, torch.float32, 2e-5)])
@pytest.mark.parametrize("with_delta", [True, False])
def test_add_layernorm_autograd_matches_torch(ops, M, D, dtype, tol, with_delta):
    """autograd.AddLayerNormFn (as_add_layernorm forward, as_add_layernorm_bwd backward) vs torch autograd in fp64 of
    x_out = x + delta, y = LayerNorm(x_out): gradients of x, delta, gamma, beta when BOTH outputs are used, with many workgroup
    partials (M = 1030: 258 workgroups, each row loop runs once) and with two workgroups (M = 5).  More rows than the 1024
    workgroups cover in one pass (M > 4096, the grid-stride loop's second pass): tests/test_gpu_layernorm.py."""
    from attentionshift_amd import autograd as AG
    g = torch.Generator().manual_seed(M + D)
    x = torch.randn(M, D, generator=g) * 2 + 0.5
    delta = (torch.randn(M, D, generator=g)).to(dtype) if with_delta else None
    gamma, beta = torch.randn(D, generator=g) * 0.3 + 1, torch.randn(D, generator=g) * 0.1
    w1, w2 = torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)
    x64, g64, b64 = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    d64 = None if delta is None else delta.double().requires_grad_(True)
    with torch.enable_grad():
        xo = x64 if d64 is None else x64 + d64
        y64 = torch.nn.functional.layer_norm(xo, (D,), g64, b64, 1e-6)
        ((xo * w1.double()).sum() + (y64 * w2.double()).sum()).backward()
    xd, gd, bd = dev(x).requires_grad_(True), dev(gamma).requires_grad_(True), dev(beta).requires_grad_(True)
    dd = None if delta is None else dev(delta).requires_grad_(True)
    with torch.enable_grad():
        xo_d, y_d = AG.add_layernorm(xd, dd, gd, bd, 1e-6, dtype)
        ((xo_d * dev(w1)).sum() + (y_d.float() * dev(w2)).sum()).backward()
    for name, ref, got in (("x_out", xo.detach(), xo_d.detach()), ("y", y64.detach(), y_d.detach()), ("dx", x64.grad, xd.grad),
                           ("dgamma", g64.grad, gd.grad), ("dbeta", b64.grad, bd.grad)) + \
            ((("ddelta", d64.grad, dd.grad),) if with_delta else ()):
        mx, mean = rel_to_range(ref.float(), got.float())
        assert mx < tol, (name, mx, mean)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.bfloat16, 2e-2)])
def test_add_layernorm_autograd_with_per_sample_delta_scale(ops, dtype, tol):
    """DropPath folded into the fused add (as_add_layernorm_scaled / _bwd_scaled): x_out = x + s[b] * delta with s = mask / keep
    per image -- forward and every gradient vs torch autograd in fp64; a dropped image (s = 0) gets ddelta = 0 exactly."""
    from attentionshift_amd import autograd as AG
    B, N, D = 3, 77, 768
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, N, D, generator=g)
    delta = torch.randn(B, N, D, generator=g).to(dtype)
    s = torch.tensor([1.0 / 0.9, 0.0, 1.0 / 0.9])
    gamma, beta = torch.randn(D, generator=g) * 0.3 + 1, torch.randn(D, generator=g) * 0.1
    w1, w2 = torch.randn(B, N, D, generator=g), torch.randn(B, N, D, generator=g)
    x64, d64 = x.double().requires_grad_(True), delta.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    with torch.enable_grad():
        xo = x64 + s.double()[:, None, None] * d64
        y64 = torch.nn.functional.layer_norm(xo, (D,), g64, b64, 1e-6)
        ((xo * w1.double()).sum() + (y64 * w2.double()).sum()).backward()
    xd, dd = dev(x).requires_grad_(True), dev(delta).requires_grad_(True)
    gd, bd = dev(gamma).requires_grad_(True), dev(beta).requires_grad_(True)
    with torch.enable_grad():
        xo_d, y_d = AG.add_layernorm(xd, dd, gd, bd, 1e-6, dtype, dev(s))
        ((xo_d * dev(w1)).sum() + (y_d.float() * dev(w2)).sum()).backward()
    for name, ref, got in (("x_out", xo.detach(), xo_d.detach()), ("y", y64.detach(), y_d.detach()), ("dx", x64.grad, xd.grad),
                           ("ddelta", d64.grad, dd.grad), ("dgamma", g64.grad, gd.grad), ("dbeta", b64.grad, bd.grad)):
        mx, mean = rel_to_range(ref.float(), got.float())
        assert mx < tol, (name, mx, mean)
    assert (dd.grad[1] == 0).all() and torch.equal(xo_d[1].detach(), xd[1].detach())


@pytest.mark.parametrize("D", [768, 1280])
def test_add_layernorm_autograd_affine_gradients_only(ops, D):
    """A first block behind a frozen token preparation: x needs no gradient, there is no delta, gamma / beta do -- the
    kernel is asked for the affine gradients alone (a scratch dx); D = 1280 (ViT-H) is beyond the 1024 of round 2."""
    from attentionshift_amd import autograd as AG
    g = torch.Generator().manual_seed(D)
    M = 300
    x = torch.randn(M, D, generator=g)
    gamma, beta = torch.randn(D, generator=g) * 0.3 + 1, torch.randn(D, generator=g) * 0.1
    w = torch.randn(M, D, generator=g)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    with torch.enable_grad():
        (torch.nn.functional.layer_norm(x.double(), (D,), g64, b64, 1e-6) * w.double()).sum().backward()
    gd, bd = dev(gamma).requires_grad_(True), dev(beta).requires_grad_(True)
    with torch.enable_grad():
        _, y = AG.add_layernorm(dev(x), None, gd, bd, 1e-6, torch.float32)
        (y * dev(w)).sum().backward()
    for name, ref, got in (("dgamma", g64.grad, gd.grad), ("dbeta", b64.grad, bd.grad)):
        mx, _ = rel_to_range(ref.float(), got.float())
        assert mx < 2e-5, (name, mx)


def test_roi_align_trainable_map_outside_the_hip_backward_limits_takes_the_tensor_path(ops):
    """mil_head.roi_align: a trainable map the HIP backward cannot take (C % 8 != 0) must not pass the forward and then
    fail in backward -- it runs on the tensor-op path, and agrees with the HIP forward of the same (no-grad) input."""
    from attentionshift_amd.mil_head import roi_align
    g = torch.Generator().manual_seed(5)
    feat = torch.randn(1, 12, 20, 24, generator=g)
    rois = torch.tensor([[0, 16.0, 20.0, 200.0, 180.0], [0, 100.0, 40.0, 330.0, 300.0]])
    fd = dev(feat).requires_grad_(True)
    with torch.enable_grad():
        y = roi_align(fd, dev(rois), 7, 1.0 / 16, 0, True)
        y.square().sum().backward()
    assert fd.grad is not None and torch.isfinite(fd.grad).all() and fd.grad.abs().sum() > 0
    with torch.no_grad():
        y_hip = roi_align(dev(feat), dev(rois), 7, 1.0 / 16, 0, True)          # C % 4 == 0, no grad: the HIP kernel
    assert_close(y_hip.cpu(), y.detach().cpu(), 1e-5, 1e-5, "roi_align tensor path vs HIP forward")


@pytest.mark.parametrize("N,h,T,dtype", [(457, 4, 40, torch.bfloat16), (1090, 12, 100, torch.bfloat16), (457, 3, 40, torch.float32)])
def test_rollout_of_a_row_subset_equals_those_rows_of_the_full_rollout(ops, N, h, T, dtype):
    """ops.rollout_rows(states, T, rows=sel): only the selected point-token rows go through the layers below the top one
    (T <= 32 variant of the step kernel, as_rollout_pack for the fragment-major operand).  A row of R . A depends on that
    row of R alone, so the result must equal the same rows of the full roll-out BIT FOR BIT."""
    g = torch.Generator().manual_seed(N + h)
    B, D = 2, h * 64
    x = torch.randn(B, N, D, generator=g).cuda().to(dtype)
    states = []
    for l in range(3):
        wq = (torch.randn(3 * D, D, generator=g) * D ** -0.5).cuda().to(dtype)
        wp = (torch.randn(D, D, generator=g) * D ** -0.5).cuda().to(dtype)
        _, st = ops.attention_fwd(x, wq, torch.zeros(3 * D, device="cuda"), wp, torch.zeros(D, device="cuda"), h, keep_state=True)
        states.append(st)
    full = ops.rollout_rows(states, T)
    sel = torch.tensor([[3, T - 1, 0, 17, 17], [5, 6, 7, 1, 2]], device="cuda")
    sub = ops.rollout_rows(states, T, rows=sel)
    assert sub.shape == (B, 3, sel.shape[1], N)
    ref = torch.gather(full, 2, sel[:, None, :, None].expand(-1, 3, -1, N))
    assert torch.equal(sub, ref), float((sub - ref).abs().max())


@pytest.mark.parametrize("B,h,w,cin,cout", [(2, 5, 7, 96, 40), (1, 16, 16, 64, 128), (2, 64, 64, 768, 768)])
@pytest.mark.parametrize("act", ["none", "gelu"])
def test_deconv2x2_matches_conv_transpose(ops, B, h, w, cin, cout, act):
    """as_deconv2x2_fwd (one GEMM over the pixels, epilogue scattering to the interleaved NHWC pixel) vs
    F.conv_transpose2d(kernel 2, stride 2) (+ exact GELU) on the same bf16-rounded operands; includes the FPN shape."""
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.randn(B, h, w, cin, generator=g).bfloat16()
    wt = (torch.randn(cin, cout, 2, 2, generator=g) * cin ** -0.5).bfloat16()
    bias = torch.randn(cout, generator=g)
    ref = torch.nn.functional.conv_transpose2d(x.float().permute(0, 3, 1, 2), wt.float(), bias, stride=2)
    if act == "gelu":
        ref = torch.nn.functional.gelu(ref)
    w4 = wt.permute(2, 3, 1, 0).reshape(4 * cout, cin).contiguous()
    got = ops.deconv2x2(dev(x), dev(w4), dev(bias.repeat(4)), act=act)
    assert got.shape == (B, 2 * h, 2 * w, cout) and got.dtype == torch.bfloat16
    mx, mean = rel_to_range(ref.permute(0, 2, 3, 1), got.float())
    assert mx < 1e-2 and mean < 1e-3, (mx, mean)


@pytest.mark.parametrize("H,W,heads,shift", [(14, 14, 2, 0), (14, 14, 4, 3), (16, 23, 3, 3), (9, 30, 8, 0), (37, 5, 5, 6)])
def test_window_attention_mfma_matches_the_fp32_kernel(ops, H, W, heads, shift):
    """bf16 tensors take the MFMA kernel, fp32 tensors the fp32 VALU kernel (which the reference fixtures pin at 1e-4):
    same bf16-rounded inputs through both -- outputs, and the softmax itself, for shifted / padded / ragged grids,
    head counts that do not fill a 4-wave workgroup, with and without the qkv bias."""
    g = torch.Generator().manual_seed(H * 100 + W + shift)
    B, C = 2, heads * 32
    qkv = (torch.randn(B, H, W, 3 * C, generator=g) * 1.5).bfloat16()
    bias = torch.randn(3 * C, generator=g) * 0.5
    table = torch.randn(169, heads, generator=g)
    for b_qkv in (bias, None):
        bq = None if b_qkv is None else dev(b_qkv)
        zeros = dev(torch.zeros(3 * C))
        ref_o, ref_a = ops.window_attention_fwd(dev(qkv.float()), zeros if bq is None else bq, dev(table), heads, 7, shift,
                                                return_attn=True)
        for want in (True, False):
            o, a = ops.window_attention_fwd(dev(qkv), zeros if bq is None else bq, dev(table), heads, 7, shift,
                                            return_attn=want)
            assert o.dtype == torch.bfloat16
            mx, mean = rel_to_range(ref_o.cpu(), o.float().cpu())
            assert mx < 2e-2 and mean < 2e-3, (H, W, heads, shift, want, mx, mean)
            if want:
                assert float((a - ref_a).abs().max()) < 2e-2
                assert float((a.sum(-1) - 1).abs().max()) < 1e-5


def test_mask_count_matches_torch(ops):
    g = torch.Generator().manual_seed(4)
    for (M, HW) in ((3, 1024 * 1024), (7, 4096), (1, 16), (5, 208)):
        mask = torch.rand(M, HW, generator=g) < 0.3
        mask[0] = False
        got = ops.mask_count(dev(mask))
        assert_equal(mask.sum(1).to(torch.int32), got, f"mask_count {M}x{HW}")


@pytest.mark.parametrize("shift", [0, 3])
def test_swin_block_config5_stage1_full_size(ops, shift):
    """BASELINE config 5 stage-1 shape (Swin-B at 1024^2: 256x256 tokens, C=128, 4 heads, window 7 -> padded to 259,
    37x37 windows per image), B=1, fp32 path, against the oracle's SwinTransformerBlock restatement (which the
    swin_*.npz fixtures pin bit-exactly to the reference)."""
    from attentionshift_amd.swin import SwinTransformerBlock
    C, heads, hw = 128, 4, 256
    g = torch.Generator().manual_seed(50 + shift)
    blk = SwinTransformerBlock(C, (hw, hw), heads, window_size=7, shift_size=shift, compute_dtype=torch.float32,
                               return_attention=False)
    with torch.no_grad():
        for n, prm in blk.named_parameters():
            prm.copy_(torch.randn(prm.shape, generator=g) * (0.5 if n.endswith("bias_table") else 0.08)
                      + (1.0 if n.endswith("norm1.weight") or n.endswith("norm2.weight") else 0.0))
    x = torch.randn(1, hw * hw, C, generator=g)
    p = {n: prm.detach() for n, prm in blk.named_parameters()}
    ref, _ = O.swin_block(x, p, heads, 7, shift)
    y, attn = blk.cuda().eval()(dev(x))
    assert attn is None
    mx, mean = rel_to_range(ref, y)
    assert mx < 1e-4, (mx, mean)


@pytest.mark.parametrize("tag", ["w14_s0", "w14_s3", "w16_s3_pad", "w9_s0_pad"])
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-4), (torch.bfloat16, 6e-2)])
def test_swin_block_backward_matches_autograd(ops, golden, tag, dtype, tol):
    """Trainable Swin block: forward + backward through WindowAttnFn (as_window_attn_fwd / as_window_attn_bwd) vs torch
    autograd (fp64) through the oracle's SwinTransformerBlock restatement: gradients of the input, the qkv weight and
    BIAS (padded tokens feed the bias), the relative-position-bias table, proj and an MLP weight."""
    from attentionshift_amd.swin import SwinTransformerBlock
    g = golden(f"swin_{tag}")
    hw, ws, heads, C, shift = int(g["hw"]), int(g["ws"]), int(g["heads"]), int(g["C"]), int(g["shift"])
    blk = SwinTransformerBlock(C, (hw, hw), heads, window_size=ws, shift_size=shift, compute_dtype=dtype)
    sd = {k[2:]: t(g[k]) for k in g.files if k.startswith("p.")}
    blk.load_state_dict(sd, strict=False)
    blk = blk.cuda().train()
    gen = torch.Generator().manual_seed(1)
    x = t(g["x"])
    w = torch.randn(x.shape, generator=gen)
    names = ["attn.qkv.weight", "attn.qkv.bias", "attn.relative_position_bias_table", "attn.proj.weight", "norm1.weight",
             "mlp.fc1.weight"]
    with torch.enable_grad():
        p64 = {k: v.double() for k, v in sd.items()}
        for n in names:
            p64[n].requires_grad_(True)
        x64 = x.double().requires_grad_(True)
        y64, _ = O.swin_block(x64, p64, heads, ws, shift)
        (y64 * w.double()).sum().backward()
        xg = dev(x).requires_grad_(True)
        y, _ = blk(xg)
        (y * dev(w)).sum().backward()
    mx, _ = rel_to_range(y64.detach().float(), y.detach().float())
    assert mx < tol, ("forward", mx)
    mx, _ = rel_to_range(x64.grad.float(), xg.grad.float())
    assert mx < tol, ("dx", mx)
    params = dict(blk.named_parameters())
    for n in names:
        assert params[n].grad is not None, n
        mx, mean = rel_to_range(p64[n].grad.float(), params[n].grad.float())
        assert mx < tol, (n, mx, mean)


@pytest.mark.parametrize("B,H,W,h,shift", [(2, 14, 14, 4, 0), (1, 14, 14, 2, 3), (1, 16, 18, 3, 3), (2, 9, 23, 1, 0),
                                            (1, 64, 64, 4, 3)])
def test_window_attention_backward_on_the_matrix_cores_matches_the_fp32_kernel(ops, B, H, W, h, shift):
    """as_window_attn_bwd on bf16 tensors (window_attn_bwd_mfma_kernel: S^T / dP^T / dQ^T, dV^T and dK^T on
    v_mfma_f32_32x32x16_bf16, P and dS through a transposing LDS read) against the fp32-arithmetic kernel fed the SAME
    bf16-rounded tensors: dqkv, the relative-position-bias-table gradient and the padded tokens' bias gradient
    (models/swin_transformer.py:131-153 under autograd; grids that need window padding and the cyclic shift included).
    Differences: P / dS rounded to bf16 before the gradient products -- 2e-2 of each output's range; twice: bitwise equal."""
    g = torch.Generator().manual_seed(H * 100 + W + shift)
    C = 32 * h
    qkv = torch.randn(B, H, W, 3 * C, generator=g).bfloat16()
    bq = torch.randn(3 * C, generator=g) * 0.2
    table = torch.randn(169, h, generator=g) * 0.5
    d_out = torch.randn(B, H, W, C, generator=g).bfloat16()
    got = ops.window_attention_bwd(dev(qkv), dev(bq), dev(table), dev(d_out), h, 7, shift)
    again = ops.window_attention_bwd(dev(qkv), dev(bq), dev(table), dev(d_out), h, 7, shift)
    ref = ops.window_attention_bwd(dev(qkv.float()), dev(bq), dev(table), dev(d_out.float()), h, 7, shift)
    for name, a, b, r in zip(("dqkv", "dtable", "dbqkv_pad"), got, again, ref):
        assert torch.equal(a, b), name
        assert torch.isfinite(a.float()).all(), name
        rng = float(r.float().abs().max())
        err = float((a.float() - r.float()).abs().max())
        assert err <= 2e-2 * rng + 1e-6, (name, err, rng)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-4), (torch.bfloat16, 6e-2)])
def test_swin_backbone_matches_reference(golden, dtype, tol):
    """The whole Swin backbone (patch embed, two stages of (shifted-)window blocks on as_window_attn_fwd, patch merging,
    final norm, pooled output) vs the reference's own SwinTransformer on a grid that needs window padding in both
    stages (30x30 and 15x15 tokens, window 7).  Same state-dict keys as the reference."""
    from attentionshift_amd import synthetic
    from attentionshift_amd.swin import SwinTransformer
    g = golden("swin_net_pad120")
    img = int(g["img"])
    net = SwinTransformer(img_size=img, patch_size=4, in_chans=3, num_classes=0, embed_dim=int(g["cfg_embed_dim"]),
                          depths=g["cfg_depths"].tolist(), num_heads=g["cfg_heads"].tolist(), window_size=7,
                          compute_dtype=dtype)
    own = net.state_dict()
    names = [k for k in own if "relative_position_index" not in k]
    assert sorted(names) == sorted(g["param_names"].tolist())
    net.load_state_dict(synthetic.det_state_dict({k: tuple(own[k].shape) for k in names}), strict=False)
    net = net.cuda().eval()
    x = torch.randn(2, 3, img, img, generator=torch.Generator().manual_seed(int(g["seed"]))).cuda()
    with torch.no_grad():
        out = net(x, return_all_tokens=True)
        _, stages = net.forward_stages(x)
    for i, s in enumerate(stages):
        ref = t(g[f"stage{i}"])
        err = float((s.float().cpu() - ref).abs().max() / ref.abs().max())
        assert err < tol, (i, err)
    ref = t(g["out"])
    assert float((out.float().cpu() - ref).abs().max() / ref.abs().max()) < tol


def test_chamfer_2d_forward_backward(ops):
    """The reference's second native op (mmdet/ops/chamfer_2d): nearest squared distances / indices by brute force in
    float64, lowest index on exact ties (integer coordinates), gradients vs autograd of the gathered form."""
    from attentionshift_amd.chamfer import Chamfer2D
    gen = torch.Generator().manual_seed(41)
    B, n, m = 3, 1300, 777                                   # more than one LDS tile, sizes 1 and 3 mod 4
    a = torch.rand(B, n, 2, generator=gen) * 100
    b = torch.rand(B, m, 2, generator=gen) * 100
    d1, d2, i1, i2 = ops.chamfer_2d_fwd(dev(a), dev(b))
    full = ((a.double()[:, :, None, :] - b.double()[:, None, :, :]) ** 2).sum(-1)             # [B,n,m]
    assert_close(full.min(2)[0], d1, 1e-5, 1e-6, "dist1"); assert_close(full.min(1)[0], d2, 1e-5, 1e-6, "dist2")
    got1 = torch.gather(full, 2, i1.cpu().long()[..., None])[..., 0]
    assert_close(full.min(2)[0], got1, 1e-5, 1e-6, "idx1 points at a nearest neighbour")
    got2 = torch.gather(full, 1, i2.cpu().long()[:, None, :])[:, 0]
    assert_close(full.min(1)[0], got2, 1e-5, 1e-6, "idx2 points at a nearest neighbour")
    # exact ties: integer grid, duplicated points -> the lowest index wins (exact arithmetic)
    ai = torch.tensor([[[0., 0.], [5., 5.], [2., 1.]]])
    bi = torch.tensor([[[1., 0.], [0., 1.], [5., 5.], [5., 5.], [-1., 0.]]])
    _, _, t1, t2 = ops.chamfer_2d_fwd(dev(ai), dev(bi))
    assert t1.tolist() == [[0, 2, 0]] and t2.tolist() == [[0, 0, 1, 1, 0]]
    # backward
    with torch.enable_grad():
        x1, x2 = dev(a).requires_grad_(True), dev(b).requires_grad_(True)
        o1, o2, j1, j2 = Chamfer2D()(x1, x2)
        w1, w2 = dev(torch.rand(B, n, generator=gen)), dev(torch.rand(B, m, generator=gen))
        ((o1 * w1).sum() + (o2 * w2).sum()).backward()
        y1, y2 = dev(a).double().requires_grad_(True), dev(b).double().requires_grad_(True)
        r1 = ((y1 - torch.gather(y2, 1, j1.long()[..., None].expand(-1, -1, 2))) ** 2).sum(-1)
        r2 = ((y2 - torch.gather(y1, 1, j2.long()[..., None].expand(-1, -1, 2))) ** 2).sum(-1)
        ((r1 * w1.double()).sum() + (r2 * w2.double()).sum()).backward()
    assert_close(y1.grad, x1.grad, 1e-4, 1e-4, "grad xyz1"); assert_close(y2.grad, x2.grad, 1e-4, 1e-4, "grad xyz2")
    # the backward is a fixed-order gather (no atomics): bitwise reproducible, also with many points sharing a neighbour
    b_few = dev(b[:, :7].contiguous())                          # 1300 points compete for 7 neighbours
    d1f, d2f, i1f, i2f = ops.chamfer_2d_fwd(dev(a), b_few)
    g1, g2 = dev(torch.rand(B, n, generator=gen)), dev(torch.rand(B, 7, generator=gen))
    first = ops.chamfer_2d_bwd(dev(a), b_few, g1, g2, i1f, i2f)
    for _ in range(3):
        again = ops.chamfer_2d_bwd(dev(a), b_few, g1, g2, i1f, i2f)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


def _ref_small_attn(qkv):
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3).double() for i in range(3))                  # [B,h,N,d]
    p = torch.softmax(q @ k.transpose(-1, -2) * q.shape[-1] ** -0.5, dim=-1)
    return (p @ v).permute(0, 2, 1, 3).flatten(2)


def _check_small_attention(ops, N, h, dtype, tol):
    gen = torch.Generator().manual_seed(N)
    Bp = 5
    qkv = (torch.randn(Bp, N, 3, h, 32, generator=gen) * 1.5).to(dtype)
    out, lse = ops.small_attention_fwd(dev(qkv))
    with torch.enable_grad():
        x = qkv.double().requires_grad_(True)
        ref = _ref_small_attn(x)
        g = torch.randn(Bp, N, h * 32, generator=gen).to(dtype)
        (ref * g.double()).sum().backward()
    rng = float(ref.abs().max())
    assert float((out.double().cpu() - ref.detach()).abs().max()) < tol * rng
    q, k = qkv[:, :, 0].permute(0, 2, 1, 3).double(), qkv[:, :, 1].permute(0, 2, 1, 3).double()
    want_lse = torch.logsumexp(q @ k.transpose(-1, -2) * 32 ** -0.5, dim=-1)
    assert_close(want_lse, lse, 1e-4 if dtype == torch.float32 else 1e-2, 1e-4 if dtype == torch.float32 else 1e-2, "lse")
    dqkv = ops.small_attention_bwd(dev(qkv), out, dev(g), lse)
    gr = float(x.grad.abs().max())
    assert float((dqkv.double().cpu() - x.grad).abs().max()) < (5 * tol) * gr


@pytest.mark.parametrize("N,dtype,tol", [(50, torch.float32, 2e-5), (197, torch.float32, 2e-5), (50, torch.bfloat16, 2e-2),
                                         (300, torch.bfloat16, 2e-2), (1, torch.float32, 2e-5),
                                         (32, torch.float32, 2e-5), (33, torch.float32, 2e-5), (64, torch.float32, 2e-5),
                                         (32, torch.bfloat16, 2e-2), (33, torch.bfloat16, 2e-2), (64, torch.bfloat16, 2e-2)])
def test_small_attention_forward_backward(ops, N, dtype, tol):
    """as_small_attn_fwd / _bwd (head dim 32, packed qkv) vs fp64 softmax attention and its autograd gradient.  N = 32, 33, 64:
    exactly one 32-row block, one row past it, exactly two."""
    _check_small_attention(ops, N, 8, dtype, tol)


@pytest.mark.parametrize("h", [1, 3])
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.bfloat16, 2e-2)])
def test_small_attention_with_a_wave_task_count_that_is_no_multiple_of_four(ops, h, dtype, tol):
    """N = 50 with h heads: 2 h wave tasks per image (two 32-row blocks x h heads) = 2 and 6, no multiple of the four waves of a
    workgroup, so the last workgroup's early-return waves run.  Same reference and tolerances."""
    _check_small_attention(ops, 50, h, dtype, tol)


def test_mae_box_head_matches_tensor_op_decoder():
    """MAEBoxHeadRec (reference parameter names) on the HIP small-N attention vs the same weights through
    torch's scaled_dot_product_attention, forward and parameter gradients."""
    import attentionshift_amd as A
    torch.manual_seed(5)
    head = A.build_head(dict(type="MAEBoxHeadRec", in_channels=96, img_size=224, patch_size=16, embed_dim=64, depth=2,
                             num_heads=2, mlp_ratio=4., num_classes=20, with_reconstruct=False, pretrained=True,
                             use_checkpoint=False, rec_weight=1.0)).cuda()
    keys = set(head.state_dict())
    assert {"det_token", "decoder_pos_embed", "norm.weight", "decoder_embed.weight", "decoder_blocks.1.attn.qkv.bias",
            "decoder_blocks.0.mlp.fc2.weight", "decoder_box_norm.bias", "fc_cls.weight", "fc_reg.bias"} <= keys
    torch.nn.init.normal_(head.decoder_pos_embed, std=0.02)
    x = torch.randn(6, 96, 7, 7).cuda()
    with torch.enable_grad():
        cls, reg, rec = head(x)
        assert cls.shape == (6, 21) and reg.shape == (6, 80) and rec is None
        (cls.square().sum() + reg.square().sum()).backward()
        got = {n: p.grad.clone() for n, p in head.named_parameters() if p.grad is not None}
        head.zero_grad()

        def ref_attn(self, t):
            B, N, C = t.shape
            qkv = self.qkv(t).reshape(B, N, 3, self.num_heads, 32).permute(2, 0, 3, 1, 4)
            o = torch.nn.functional.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2])
            return self.proj(o.transpose(1, 2).reshape(B, N, C))

        from attentionshift_amd import mae_heads
        orig = mae_heads._Attention.forward
        mae_heads._Attention.forward = ref_attn
        try:
            cls2, reg2, _ = head(x)
            (cls2.square().sum() + reg2.square().sum()).backward()
        finally:
            mae_heads._Attention.forward = orig
    assert_close(cls2, cls, 1e-4, 1e-5, "cls_score"); assert_close(reg2, reg, 1e-4, 1e-5, "bbox_pred")
    for n, p in head.named_parameters():
        if p.grad is not None:
            assert_close(p.grad, got[n], 2e-3, 1e-5, f"grad {n}")


@pytest.mark.parametrize("kind", ["box", "mask"])
def test_mae_heads_bf16_training_path_matches_the_library_path(kind, monkeypatch):
    """Under bf16 autocast the heads' layers run on autograd.LinearFn (as_linear_fwd / as_linear_bwd) and the blocks'
    residual adds + LayerNorms on autograd.AddLayerNormFn; the same weights with every nn.Linear / LayerNorm left to the
    library under the same autocast region must agree to bf16 rounding, outputs and parameter gradients."""
    import attentionshift_amd as A
    from attentionshift_amd import autograd as AG
    torch.manual_seed(11)
    common = dict(in_channels=96, img_size=224, patch_size=16, embed_dim=256, depth=2, num_heads=8, mlp_ratio=4., num_classes=20)
    if kind == "box":
        head = A.build_head(dict(type="MAEBoxHeadRec", with_reconstruct=False, **common)).cuda()
        x = torch.randn(48, 96, 7, 7).cuda()
    else:
        head = A.build_head(dict(type="MAEMaskHeadPointSup", scale_factor=2, scale_mode="bicubic", **common)).cuda()
        x = torch.randn(12, 96, 14, 14).cuda()
    torch.nn.init.normal_(head.decoder_pos_embed, std=0.02)
    head.train()

    def run():
        head.zero_grad()
        xin = x.clone().requires_grad_(True)
        with torch.enable_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            out = head(xin)
            outs = [o for o in (out if isinstance(out, tuple) else (out,)) if o is not None]
            sum(o.float().square().mean() for o in outs).backward()
        return [o.detach().float() for o in outs], xin.grad, {n: p.grad.clone() for n, p in head.named_parameters() if p.grad is not None}

    calls, blocks = [], []
    orig, orig_blk = AG.LinearFn.forward, AG.DecoderBlockFn.forward
    monkeypatch.setattr(AG.LinearFn, "forward", staticmethod(lambda ctx, *a: (calls.append(1), orig(ctx, *a))[1]))
    monkeypatch.setattr(AG.DecoderBlockFn, "forward", staticmethod(lambda ctx, *a: (blocks.append(1), orig_blk(ctx, *a))[1]))
    outs, dx, grads = run()
    # decoder_embed (+ the box head's output layers) through LinearFn, the two decoder blocks as one fused node each
    # (DecoderBlockFn: the same as_linear_fwd / as_linear_bwd kernels for their four layers)
    assert len(calls) >= 1 and len(blocks) == 2, ("the HIP linear path did not run", len(calls), len(blocks))
    monkeypatch.setattr(AG, "_LIBRARY_LINEAR", True)
    n_before, b_before = len(calls), len(blocks)
    outs2, dx2, grads2 = run()
    assert len(calls) == n_before and len(blocks) == b_before, "the library path still went through the HIP bridges"
    for a, b in zip(outs2, outs):
        mx, mean = rel_to_range(a, b)
        assert mx < 4e-2 and mean < 5e-3, ("output", mx, mean)
    mx, mean = rel_to_range(dx2, dx)
    assert mx < 6e-2 and mean < 6e-3, ("dx", mx, mean)
    assert set(grads) == set(grads2)
    for n in grads:
        mx, mean = rel_to_range(grads2[n], grads[n])
        assert mx < 8e-2 and mean < 1e-2, (n, mx, mean)


@pytest.mark.parametrize("autocast", [False, True])
def test_mae_heads_take_an_empty_roi_batch(autocast):
    """No positive RoIs in a batch (images without objects): the heads run on [0, C, h, w] as the reference's modules
    do, the loss is 0 and every parameter still gets a (zero) gradient."""
    import attentionshift_amd as A
    common = dict(in_channels=96, img_size=224, patch_size=16, embed_dim=256, depth=1, num_heads=8, mlp_ratio=4., num_classes=20)
    mask = A.build_head(dict(type="MAEMaskHeadPointSup", scale_factor=2, scale_mode="bicubic", **common)).cuda().train()
    box = A.build_head(dict(type="MAEBoxHeadRec", with_reconstruct=False, **common)).cuda().train()
    with torch.enable_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        pred = mask(torch.zeros(0, 96, 14, 14).cuda())
        assert pred.shape == (0, 20, 28, 28)
        loss = mask.loss(pred, torch.zeros(0, 5, device="cuda"), torch.zeros(0, dtype=torch.long, device="cuda"))["loss_mask"]
        cls, reg, _ = box(torch.zeros(0, 96, 7, 7).cuda())
        assert cls.shape == (0, 21) and reg.shape == (0, 80)
        (loss + cls.sum() + reg.sum()).backward()
    assert float(loss) == 0.0
    for head in (mask, box):
        missing = [n for n, p in head.named_parameters() if p.requires_grad and p.grad is None and "pos_embed" not in n]
        assert not missing, missing


def test_mae_mask_head_forward_loss_and_gradients():
    """MAEMaskHeadPointSup on the HIP small-N attention (196 tokens per RoI) vs the same weights through torch's
    scaled_dot_product_attention; point-sampled BCE loss with ignored points; gradients reach every parameter."""
    import attentionshift_amd as A
    from attentionshift_amd import mae_heads, mask_targets as MT
    torch.manual_seed(9)
    head = A.build_head(dict(type="MAEMaskHeadPointSup", in_channels=48, img_size=224, patch_size=16, embed_dim=64,
                             depth=2, num_heads=2, mlp_ratio=4., num_classes=20, scale_factor=2, scale_mode="bicubic",
                             use_checkpoint=False, init_cfg=None)).cuda()
    torch.nn.init.normal_(head.decoder_pos_embed, std=0.02)
    assert {"decoder_blocks.1.attn.proj.weight", "conv_logits.weight", "decoder_embed.bias", "decoder_box_norm.weight"} <= set(head.state_dict())
    x = torch.randn(5, 48, 14, 14).cuda()
    sites = torch.rand(5, 12, 2).cuda()
    targets = torch.randint(0, 3, (5, 12)).cuda()
    labels = torch.tensor([0, 3, 19, 7, 7]).cuda()

    def run():
        pred = head(x)
        assert pred.shape == (5, 20, 28, 28)
        return pred, head.loss(MT.point_sample(pred, sites), targets, labels)["loss_mask"]

    def ref_attn(self, t):
        B, N, C = t.shape
        qkv = self.qkv(t).reshape(B, N, 3, self.num_heads, 32).permute(2, 0, 3, 1, 4)
        o = torch.nn.functional.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2])
        return self.proj(o.transpose(1, 2).reshape(B, N, C))

    with torch.enable_grad():
        pred, loss = run()
        loss.backward()
        got = {n: p.grad.clone() for n, p in head.named_parameters() if p.grad is not None}
        head.zero_grad()
        orig = mae_heads._Attention.forward
        mae_heads._Attention.forward = ref_attn
        try:
            pred2, loss2 = run()
            loss2.backward()
        finally:
            mae_heads._Attention.forward = orig
    assert_close(pred2, pred, 1e-4, 1e-5, "mask logits"); assert_close(loss2, loss, 1e-5, 1e-6, "loss_mask")
    assert set(got) == {n for n, p in head.named_parameters() if p.requires_grad}
    for n, p in head.named_parameters():
        if p.grad is not None:
            assert_close(p.grad, got[n], 2e-3, 1e-6, f"grad {n}")


def test_mt19937_device_draws_equal_torchs_cpu_generator(ops):
    """as_mt_sample_ranks / as_mt_perm_ranks (csrc/mt19937.hip) against torch's own global CPU generator: the ranks the
    reference's `torch.randint(n, (n_draw,))` / `torch.randperm(n)[:k]` calls give (stdroi:343-371, 447), call after call
    on ONE engine state, across many refills (a 600 000-candidate permutation skips ~960 blocks), and the generator state
    torch is left in afterwards -- bit for bit."""
    from attentionshift_amd import mt19937 as MT
    rng = np.random.default_rng(4)
    torch.manual_seed(2024)
    torch.rand(333)                                         # start somewhere inside a block
    start = torch.get_rng_state()
    state = torch.from_numpy(MT.unpack_state(start).copy()).cuda()
    for rep in range(3):
        S, K, G, KP = 7, 20, 4, 10
        counts = rng.integers(20, 60000, S).astype(np.int32)
        counts[rep] = 20 + rep                               # n // k == 1: the longest draw lists
        counts2 = np.stack((rng.integers(0, 30000, G), rng.integers(5, 40000, G)), 1).astype(np.int32)
        counts2[0] = (10, 0) if rep == 0 else (300000, 300000)
        want_s = [(torch.randint(int(n), (len(range(0, int(n), int(n) // K)),)) % int(n))[:K].tolist() for n in counts]
        want_p = [torch.randperm(int(a + b))[:KP].tolist() for a, b in counts2]
        ranks, flag = ops.mt_sample_ranks(state, torch.from_numpy(counts).cuda(), K)
        perm, flag2 = ops.mt_perm_ranks(state, torch.from_numpy(counts2).cuda(), KP)
        assert int(flag) == 0 and int(flag2) == 0
        assert ranks.cpu().tolist() == want_s, rep
        assert perm.cpu().tolist() == want_p, rep
    assert torch.equal(MT.pack_state(start, state.cpu().numpy()), torch.get_rng_state())
    # sets the host must handle are flagged
    _, f = ops.mt_sample_ranks(state, torch.tensor([500, 19, 40], dtype=torch.int32).cuda(), 20)
    _, f2 = ops.mt_perm_ranks(state, torch.tensor([[4, 5], [100, 100]], dtype=torch.int32).cuda(), 10)
    assert int(f) != 0 and int(f2) != 0


@pytest.mark.parametrize("M,D,H", [(8394, 768, 3072), (197, 256, 1024), (50, 64, 128), (1, 32, 32), (2051, 1024, 4096)])
def test_mlp_with_the_gelu_in_the_gemm_epilogues(ops, M, D, H):
    """autograd.MlpFn's kernels (models/vision_transformer.py:47-59 under autograd).
    as_linear_gelu_fwd: the pre-activation it writes is as_linear_fwd's output bit for bit, and the activation is the erf-GELU
    of that bf16 tensor (fp64 reference, half a bf16 ulp + the 1.5e-7 of the erf polynomial);
    as_linear_bwd_dgelu: dx equals GeluBackward(as_linear_bwd's dx, pre) computed in fp64 from the SAME bf16 tensors to a
    bf16 ulp, dW / db are as_linear_bwd's bit for bit;
    MlpFn end to end against fp64 autograd of fc2(gelu(fc1(x))) on the rounded operands (3e-2 of each gradient's range)."""
    from attentionshift_amd import autograd as AG
    g = torch.Generator().manual_seed(M + D)
    x = torch.randn(M, D, generator=g).bfloat16()
    w1 = (torch.randn(H, D, generator=g) / D ** 0.5).bfloat16()
    b1 = torch.randn(H, generator=g) * 0.5
    w2 = (torch.randn(D, H, generator=g) / H ** 0.5).bfloat16()
    b2 = torch.randn(D, generator=g) * 0.1
    dy = torch.randn(M, D, generator=g).bfloat16()
    a, pre = ops.linear_gelu(dev(x), dev(w1), dev(b1))
    assert torch.equal(pre, ops.linear(dev(x), dev(w1), dev(b1)))
    ref_a = torch.nn.functional.gelu(pre.cpu().double())
    assert float((a.cpu().double() - ref_a).abs().max()) <= 2 ** -8 * float(ref_a.abs().max()) + 1e-6
    # backward of fc2 with the GELU derivative in the epilogue
    dpre, dw2, db2 = ops.linear_bwd(a, dev(w2), dev(dy), True, True, True, dw_dtype=torch.float32, gelu_pre=pre)
    da, dw2u, db2u = ops.linear_bwd(a, dev(w2), dev(dy), True, True, True, dw_dtype=torch.float32)
    assert torch.equal(dw2, dw2u) and torch.equal(db2, db2u)
    h64 = pre.cpu().double()
    dgelu = 0.5 * (1 + torch.erf(h64 / 2 ** 0.5)) + h64 * torch.exp(-h64 * h64 / 2) / (2 * torch.pi) ** 0.5
    ref_dpre = da.cpu().double() * dgelu
    assert float((dpre.cpu().double() - ref_dpre).abs().max()) <= 2 ** -8 * float(ref_dpre.abs().max()) + 1e-6
    # the autograd node end to end
    with torch.enable_grad():
        xs, w1s, b1s, w2s, b2s = (dev(t).requires_grad_(True) for t in (x, w1.float(), b1, w2.float(), b2))
        y = AG.mlp(xs, w1s, b1s, w2s, b2s)
        y.backward(dev(dy))
        x64, w164, b164, w264, b264 = (t.double().requires_grad_(True) for t in (x, w1, b1, w2, b2))
        y64 = torch.nn.functional.linear(torch.nn.functional.gelu(torch.nn.functional.linear(x64, w164, b164)), w264, b264)
        y64.backward(dy.double())
    mx, _ = rel_to_range(y64.detach().float(), y.float())
    assert mx < 3e-2, mx
    for name, got, ref in (("dx", xs.grad, x64.grad), ("dw1", w1s.grad, w164.grad), ("db1", b1s.grad, b164.grad),
                           ("dw2", w2s.grad, w264.grad), ("db2", b2s.grad, b264.grad)):
        mx, _ = rel_to_range(ref.float(), got.float())
        assert mx < 3e-2, (name, mx)
    assert w1s.grad.dtype == torch.float32 and b1s.grad.dtype == torch.float32


@pytest.mark.parametrize("M,K,Nout", [(8394, 768, 3072), (8394, 3072, 768), (2051, 256, 1024), (4197, 128, 256)])
def test_weight_gradient_without_transposes_equals_the_transposed_path(ops, M, K, Nout):
    """as_linear_bwd's two weight-gradient routes -- row-major activations through the transposing LDS read (default) and
    the round-3 route through transposed, zero-padded copies (AS_BWD_TRANSPOSED=1, read once per process: a child process)
    -- against each other and against fp64: the same products, summed in different orders (fp32 partial tiles: 1e-3 of the
    range apart at most), bias gradients included; the transpose-free route twice: bitwise reproducible."""
    import subprocess, sys, os, json
    g = torch.Generator().manual_seed(M + K)
    x = torch.randn(M, K, generator=g).bfloat16()
    w = (torch.randn(Nout, K, generator=g) / K ** 0.5).bfloat16()
    dy = torch.randn(M, Nout, generator=g).bfloat16()
    dx, dw, db = ops.linear_bwd(dev(x), dev(w), dev(dy), True, True, True, dw_dtype=torch.float32)
    dx2, dw2, db2 = ops.linear_bwd(dev(x), dev(w), dev(dy), True, True, True, dw_dtype=torch.float32)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    ref_dw = dy.double().t() @ x.double()
    ref_db = dy.double().sum(0)
    assert float((dw.cpu().double() - ref_dw).abs().max()) <= 2e-5 * float(ref_dw.abs().max()) + 1e-6 * M ** 0.5
    assert float((db.cpu().double() - ref_db).abs().max()) <= 2e-5 * float(ref_db.abs().max()) + 1e-6 * M ** 0.5
    code = (
        "import sys, json, torch; sys.path.insert(0, %r)\n"
        "from attentionshift_amd import ops\n"
        "g = torch.Generator().manual_seed(%d)\n"
        "x = torch.randn(%d, %d, generator=g).bfloat16(); w = (torch.randn(%d, %d, generator=g) / %d ** 0.5).bfloat16()\n"
        "dy = torch.randn(%d, %d, generator=g).bfloat16()\n"
        "dx, dw, db = ops.linear_bwd(x.cuda(), w.cuda(), dy.cuda(), True, True, True, dw_dtype=torch.float32)\n"
        "torch.save((dw.cpu(), db.cpu()), %r)\n"
    ) % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), M + K, M, K, Nout, K, K, M, Nout, "/tmp/as_tn_ref_%d_%d.pt" % (M, K))
    cp = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, AS_BWD_TRANSPOSED="1"), capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0, cp.stderr[-2000:]
    dw_t, db_t = torch.load("/tmp/as_tn_ref_%d_%d.pt" % (M, K))
    assert float((dw.cpu() - dw_t).abs().max()) <= 1e-3 * float(dw_t.abs().max())
    assert float((db.cpu() - db_t).abs().max()) <= 1e-3 * float(db_t.abs().max()) + 1e-4
