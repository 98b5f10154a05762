"""Every instantiation of the fused residual add + LayerNorm kernels (csrc/layernorm.hip) against fp64.

`launch_add_ln` picks `add_layernorm_kernel<T, VPL>` with VPL = ceil(D / 256) float4 groups per lane (1..8, then 10 for
9..10 and 12 for 11..12); `launch_add_ln_bwd` picks `add_layernorm_bwd_kernel<T, VPL>` for VPL 1..8.  The D lists below
take, for every lane-group count, the width that leaves one live float4 in the last group (`c < D` true for lane 0 only) and
the full one, both limits (3072 forward, 2048 backward) and the rejection past them; the backward also runs with more rows
than its 1024 workgroups x 4 waves cover in one pass (M = 4103: a second grid-stride pass of seven rows), and with 50
partials (M = 197: the remainder loop of the reduce kernel).

Tolerances: the project's own (test_gpu_kernels.py) -- forward y 2e-6 of the range in fp32 and 1e-2 in bf16, gradients 2e-5
and 2e-2.  Where a case cannot be expected to keep them the bound does not come from the kernel: the same quantity is
computed with torch on the host in fp32 (for bf16: fp32, then the roundings the op's dtype implies), its error against the
fp64 reference is measured, and max(project tolerance, 4 x that error) is allowed -- 4 for a different but equally valid
fp32 summation order.  Largest host error measured over the cases of this file (`_host_error_report()`, of the range):
    fp32 forward y                       1.9e-7  (bound stays 2e-6)
    fp32 forward y, x = randn * 3 + 1000 1.02e-5 (bound 4.1e-5: the fp32 sum of ~1000-sized terms moves the mean by ~1e-4
                                                  of a spread of 3; the kernel's lane-then-butterfly order, emulated in
                                                  numpy fp32 on the same rows, gives 0.4e-5 .. 1.1e-5)
    fp32 gradients                       5.4e-7  (bound stays 2e-5)
    bf16 forward y                       3.6e-3  (bound 1.5e-2: half a bf16 ulp at the top of the range is 3.9e-3 of it)
    bf16 gradients                       6.6e-3  (bound 2.6e-2 at most: dy and ddelta are rounded to bf16)
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

BF16, F32 = torch.bfloat16, torch.float32
FWD_D = [4, 256, 260, 512, 516, 772, 1028, 1284, 1536, 1540, 1792, 1796, 2048, 2052, 2304, 2308, 2560, 2564, 2816, 2820, 3072]
BWD_D = [4, 256, 260, 512, 516, 772, 1028, 1284, 1536, 1540, 1792, 1796, 2048]
ADD_ONLY_D = {256: 1, 260: 2, 516: 3, 772: 4, 1028: 5, 1284: 6, 1540: 7, 1796: 8, 2052: 10, 2564: 12}    # D -> instantiation
FWD_TOL = {F32: 2e-6, BF16: 1e-2}
BWD_TOL = {F32: 2e-5, BF16: 2e-2}


def fwd_vpl(D):
    """launch_add_ln's switch: the VPL instantiated for width D"""
    v = -(-D // 256)
    return v if v <= 8 else {9: 10, 10: 10, 11: 12, 12: 12}[v]


def test_parameter_lists_reach_every_instantiation():
    assert {fwd_vpl(D) for D in FWD_D} == {1, 2, 3, 4, 5, 6, 7, 8, 10, 12}
    assert {-(-D // 256) for D in FWD_D} == set(range(1, 13))            # the rounded-up 9 and 11 too
    assert {-(-D // 256) for D in BWD_D} == set(range(1, 9))
    assert {fwd_vpl(D) for D in ADD_ONLY_D} == {1, 2, 3, 4, 5, 6, 7, 8, 10, 12} and all(fwd_vpl(D) == v for D, v in ADD_ONLY_D.items())
    for v in range(1, 13):                                               # per lane-group count: one live float4 in the last group
        assert (v - 1) * 256 + 4 in FWD_D and (v > 8 or (v - 1) * 256 + 4 in BWD_D), v
    assert max(FWD_D) == 3072 and max(BWD_D) == 2048


@pytest.fixture(scope="module")
def ops():
    from attentionshift_amd import ops as _ops
    _ops._lib.load()
    return _ops


def dev(x):
    return None if x is None else x.cuda().contiguous()


def rel_to_range(ref, got):
    ref, got = ref.double().cpu(), got.double().cpu()
    scale = ref.abs().max().item() + 1e-30
    return (ref - got).abs().max().item() / scale


def y_bound(x_in, gamma, beta, dtype):
    """-> (fp64 LayerNorm of x_in, allowed max error of the range): max(project tolerance, 4 x the error of F.layer_norm in
    fp32 on the host, rounded to `dtype`)"""
    D = x_in.shape[-1]
    ref = F.layer_norm(x_in.double(), (D,), gamma.double(), beta.double(), 1e-6)
    host = F.layer_norm(x_in, (D,), gamma, beta, 1e-6).to(dtype).float()
    e = rel_to_range(ref, host)
    return ref, max(FWD_TOL[dtype], 4 * e), e


def _fwd_inputs(M, D, dtype, offset=0.5, seed=0):
    g = torch.Generator().manual_seed(7 * M + D + seed)
    x = torch.randn(M, D, generator=g) * 3 + offset
    delta = torch.randn(M, D, generator=g).to(dtype)
    gamma, beta = torch.randn(D, generator=g) * 0.2 + 1.0, torch.randn(D, generator=g) * 0.1
    return x, delta, gamma, beta


def _check_forward(ops, M, D, dtype, offset=0.5):
    x, delta, gamma, beta = _fwd_inputs(M, D, dtype, offset)
    x_ref = x + delta.float()
    x_new, y = ops.add_layernorm(dev(x), dev(delta), dev(gamma), dev(beta), 1e-6, dtype)             # add + LN
    assert y.dtype == dtype and torch.equal(x_new.cpu(), x_ref), "x + delta must be exact in fp32"
    ref, tol, e = y_bound(x_ref, gamma, beta, dtype)
    mx = rel_to_range(ref, y.float())
    print("ln fwd", dtype, M, D, offset, "add+LN err %.3g (host fp32 %.3g, bound %.3g)" % (mx, e, tol))
    assert torch.isfinite(y.float()).all() and mx < tol, (mx, tol)
    _, y0 = ops.add_layernorm(dev(x), None, dev(gamma), dev(beta), 1e-6, dtype)                      # LN only
    ref, tol, e = y_bound(x, gamma, beta, dtype)
    mx = rel_to_range(ref, y0.float())
    print("ln fwd", dtype, M, D, offset, "LN only err %.3g (host fp32 %.3g, bound %.3g)" % (mx, e, tol))
    assert torch.isfinite(y0.float()).all() and mx < tol, (mx, tol)
    if D in ADD_ONLY_D:                                                                              # add only
        x_only, none = ops.add_layernorm(dev(x), dev(delta), None, None, 0.0, dtype, want_y=False)
        assert none is None and torch.equal(x_only.cpu(), x_ref)


@pytest.mark.parametrize("D", FWD_D)
@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_add_layernorm_every_instantiation(ops, dtype, M, D):
    """add + LN, LN only and (one D per instantiation) add only: x_out = x + delta bit for bit, y against F.layer_norm in fp64
    on that x_out.  M = 1 leaves three waves of the only workgroup without a row, M = 5 three waves of the second."""
    _check_forward(ops, M, D, dtype)


@pytest.mark.parametrize("D", [260, 3072])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_add_layernorm_with_a_large_common_offset(ops, dtype, D):
    """x = randn * 3 + 1000: the variance is 1e-5 of the mean square, so a one-pass E[x^2] - E[x]^2 in fp32 (error ~6e-8 * 1e6
    against a variance of 9) loses the result; the two-pass form the kernel documents keeps it."""
    _check_forward(ops, 5, D, dtype, offset=1000.0)


def test_add_layernorm_rejects_unsupported_widths(ops):
    from attentionshift_amd._lib import AttnShiftError
    for D, rc in ((3076, "rc=-2"), (6, "rc=-1")):                        # AS_E_UNSUPPORTED past 3072; AS_E_BADARG for D % 4 != 0
        x, delta, gamma, beta = _fwd_inputs(5, D, F32)
        with pytest.raises(AttnShiftError, match=rc):
            ops.add_layernorm(dev(x), dev(delta), dev(gamma), dev(beta), 1e-6, F32)
        torch.cuda.synchronize()


@pytest.mark.parametrize("D", [260, 3072])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_add_layernorm_scaled_forward(ops, dtype, D):
    """as_add_layernorm_scaled: x_out = x + s[b] * delta with 7 rows per image (a workgroup's four rows straddle images)."""
    B, N = 3, 7
    x, delta, gamma, beta = _fwd_inputs(B * N, D, dtype, seed=3)
    x, delta = x.reshape(B, N, D), delta.reshape(B, N, D)
    s = torch.tensor([1.0 / 0.9, 0.0, 0.37])
    x_new, y = ops.add_layernorm(dev(x), dev(delta), dev(gamma), dev(beta), 1e-6, dtype, delta_scale=dev(s))
    want = x.double() + s.double()[:, None, None] * delta.double()
    assert rel_to_range(want, x_new) < 2e-7                               # one fp32 rounding (an fma) of the exact value
    assert torch.equal(x_new[1].cpu(), x[1])                              # the dropped image
    ref, tol, e = y_bound(x_new.cpu(), gamma, beta, dtype)
    mx = rel_to_range(ref, y.float())
    print("ln fwd scaled", dtype, D, "err %.3g (host fp32 %.3g, bound %.3g)" % (mx, e, tol))
    assert mx < tol, (mx, tol)


# ------------------------------------------------------------------------------------------------
# backward
# ------------------------------------------------------------------------------------------------
def _bwd_inputs(M, D, dtype, with_delta):
    g = torch.Generator().manual_seed(3 * M + D)
    x = torch.randn(M, D, generator=g) * 2 + 0.5
    delta = torch.randn(M, D, generator=g).to(dtype) if with_delta else None
    gamma, beta = torch.randn(D, generator=g) * 0.3 + 1, torch.randn(D, generator=g) * 0.1
    w1, w2 = torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)
    return x, delta, gamma, beta, w1, w2


def _host_grads(x, delta, gamma, beta, w1, w2, prec, srow=None):
    """torch autograd on the host in `prec` of loss = sum(x_out * w1) + sum(y * w2), x_out = x + srow * delta, y = LN(x_out)
    -> {name: tensor}"""
    D = x.shape[-1]
    xx, gg, bb = (t.to(prec).requires_grad_(True) for t in (x, gamma, beta))
    dd = None if delta is None else delta.to(prec).requires_grad_(True)
    with torch.enable_grad():
        xo = xx if dd is None else (xx + dd if srow is None else xx + srow.to(prec)[:, None] * dd)
        y = F.layer_norm(xo, (D,), gg, bb, 1e-6)
        loss = (y * w2.to(prec)).sum() if w1 is None else (xo * w1.to(prec)).sum() + (y * w2.to(prec)).sum()
        loss.backward()
    out = {"x_out": xo.detach(), "y": y.detach(), "dx": xx.grad, "dgamma": gg.grad, "dbeta": bb.grad}
    if dd is not None:
        out["ddelta"] = dd.grad
    return out


def _bwd_bounds(x, delta, gamma, beta, w1, w2, dtype, srow=None):
    """-> (fp64 reference, {name: allowed max error of the range}, {name: host fp32 error}).  The host fp32 evaluation
    takes what the op's dtype implies: dy (= w2) and the returned y / ddelta rounded to `dtype`."""
    ref = _host_grads(x, delta, gamma, beta, w1, w2, torch.float64, srow)
    host = _host_grads(x, delta, gamma, beta, w1, w2.to(dtype).float(), torch.float32, srow)
    tol, errs = {}, {}
    for name, r in ref.items():
        hv = host[name].to(dtype).float() if name in ("y", "ddelta") else host[name]
        errs[name] = rel_to_range(r, hv)
        proj = (FWD_TOL if name in ("x_out", "y") else BWD_TOL)[dtype]
        tol[name] = max(proj, 4 * errs[name])
    return ref, tol, errs


def _check_backward(ops, M, D, dtype, with_delta):
    from attentionshift_amd import autograd as AG
    x, delta, gamma, beta, w1, w2 = _bwd_inputs(M, D, dtype, with_delta)
    ref, tol, errs = _bwd_bounds(x, delta, gamma, beta, w1, w2, dtype)
    xd, gd, bd = dev(x).requires_grad_(True), dev(gamma).requires_grad_(True), dev(beta).requires_grad_(True)
    dd = None if delta is None else dev(delta).requires_grad_(True)
    with torch.enable_grad():
        xo_d, y_d = AG.add_layernorm(xd, dd, gd, bd, 1e-6, dtype)
        ((xo_d * dev(w1)).sum() + (y_d.float() * dev(w2)).sum()).backward()
    got = {"x_out": xo_d.detach(), "y": y_d.detach(), "dx": xd.grad, "dgamma": gd.grad, "dbeta": bd.grad}
    if with_delta:
        got["ddelta"] = dd.grad
    assert set(got) == set(ref)
    for name in ref:
        assert got[name] is not None, name
        mx = rel_to_range(ref[name], got[name].float())
        print("ln bwd", dtype, M, D, with_delta, name, "err %.3g (host fp32 %.3g, bound %.3g)" % (mx, errs[name], tol[name]))
        assert torch.isfinite(got[name].float()).all() and mx < tol[name], (name, mx, tol[name])


@pytest.mark.parametrize("with_delta", [True, False], ids=["delta", "nodelta"])
@pytest.mark.parametrize("D", BWD_D)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_add_layernorm_backward_every_instantiation(ops, dtype, D, with_delta):
    """autograd.add_layernorm (as_add_layernorm forward, as_add_layernorm_bwd backward) at M = 5 vs torch autograd in fp64:
    x_out, y, dx, ddelta, dgamma, dbeta, both outputs used."""
    _check_backward(ops, 5, D, dtype, with_delta)


@pytest.mark.parametrize("with_delta", [True, False], ids=["delta", "nodelta"])
@pytest.mark.parametrize("M,D", [(197, 260), (4103, 128), (4103, 772), (4103, 2048)])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_add_layernorm_backward_row_loop_and_partials(ops, dtype, M, D, with_delta):
    """M = 197: 50 workgroup partials = 3 rounds of the reduce kernel's 16 groups + 2 (its 4-way unrolled loop never runs, the
    remainder loop does).  M = 4103: more rows than the 1024 workgroups x 4 waves take in one pass -- rows 4096..4102 are the
    second grid-stride pass of seven waves -- and 1024 partials, the whole unrolled reduce."""
    assert -(-M // 4) == 50 or M > 4096
    _check_backward(ops, M, D, dtype, with_delta)


def test_add_layernorm_backward_affine_gradients_only(ops):
    """x needs no gradient and there is no delta: the kernel is asked for dgamma / dbeta alone (a scratch dx), VPL = 7."""
    from attentionshift_amd import autograd as AG
    M, D = 197, 1540
    x, _, gamma, beta, _, w2 = _bwd_inputs(M, D, F32, False)
    ref, tol, errs = _bwd_bounds(x, None, gamma, beta, None, w2, F32)
    gd, bd = dev(gamma).requires_grad_(True), dev(beta).requires_grad_(True)
    with torch.enable_grad():
        _, y = AG.add_layernorm(dev(x), None, gd, bd, 1e-6, F32)
        (y * dev(w2)).sum().backward()
    for name, got in (("dgamma", gd.grad), ("dbeta", bd.grad)):
        mx = rel_to_range(ref[name], got)
        print("ln bwd affine", name, "err %.3g (host fp32 %.3g, bound %.3g)" % (mx, errs[name], tol[name]))
        assert mx < tol[name], (name, mx)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_add_layernorm_backward_scaled_with_unequal_images(ops, dtype):
    """as_add_layernorm_bwd_scaled through the C ABI at M = 4103, D = 128, rows_per_scale = 1501: three images of 1501, 1501
    and 1101 rows, both image boundaries inside a workgroup's four rows; the rows of the second grid-stride pass (4096..4102)
    belong to the third image.  ddelta = s[row / 1501] * dx, exactly 0 for the dropped image."""
    import ctypes
    M, D, rps = 4103, 128, 1501
    x, delta, gamma, beta, w1, w2 = _bwd_inputs(M, D, dtype, True)
    s = torch.tensor([1.0 / 0.9, 0.0, 0.37])
    srow = s[torch.arange(M) // rps]
    ref, tol, errs = _bwd_bounds(x, delta, gamma, beta, w1, w2, dtype, srow)
    x_out = torch.addcmul(x, srow[:, None], delta.float())               # what the forward saved (fp32)
    lib = ops._lib.load()
    xo_d, dy_d, dxr_d, g_d, s_d = dev(x_out), dev(w2.to(dtype)), dev(w1), dev(gamma), dev(s)
    dx = torch.empty(M, D, device="cuda")
    ddl = torch.empty(M, D, device="cuda", dtype=dtype)
    dg, db = torch.empty(D, device="cuda"), torch.empty(D, device="cuda")
    nbytes = lib.as_add_layernorm_bwd_workspace_bytes(M, D)
    ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                          # noqa: E731
    ops._lib.check(lib.as_add_layernorm_bwd_scaled(p(xo_d), p(dy_d), p(dxr_d), p(g_d), 1e-6, p(dx), p(ddl), p(dg), p(db), p(ws),
                                                   nbytes, M, D, ops._dt(dy_d), p(s_d), rps, ops._stream()),
                   "as_add_layernorm_bwd_scaled")
    for name, got in (("dx", dx), ("ddelta", ddl), ("dgamma", dg), ("dbeta", db)):
        mx = rel_to_range(ref[name], got.float())
        print("ln bwd scaled", dtype, name, "err %.3g (host fp32 %.3g, bound %.3g)" % (mx, errs[name], tol[name]))
        assert mx < tol[name], (name, mx)
    assert (ddl[rps:2 * rps] == 0).all()                                  # the dropped image, exactly


def test_add_layernorm_backward_rejects_widths_past_2048(ops):
    """D = 2052 has a forward (VPL 9 -> <10>) but no backward instantiation: AS_E_UNSUPPORTED, not a silent truncation."""
    from attentionshift_amd import autograd as AG
    from attentionshift_amd._lib import AttnShiftError
    x, delta, gamma, beta, w1, w2 = _bwd_inputs(5, 2052, F32, True)
    xd, dd = dev(x).requires_grad_(True), dev(delta).requires_grad_(True)
    with torch.enable_grad():
        xo_d, y_d = AG.add_layernorm(xd, dd, dev(gamma), dev(beta), 1e-6, F32)
        loss = (xo_d * dev(w1)).sum() + (y_d * dev(w2)).sum()
        with pytest.raises(AttnShiftError, match="rc=-2"):
            loss.backward()
    torch.cuda.synchronize()


def _host_error_report():
    """the figures of MEASURED: largest host-fp32 error over the cases above (no device needed)"""
    out = {}
    for dtype in (F32, BF16):
        for M in (1, 5):
            for D in FWD_D:
                x, delta, gamma, beta = _fwd_inputs(M, D, dtype)
                for xin in (x + delta.float(), x):
                    out[("fwd", dtype)] = max(out.get(("fwd", dtype), 0), y_bound(xin, gamma, beta, dtype)[2])
        for D in (260, 3072):
            x, delta, gamma, beta = _fwd_inputs(5, D, dtype, 1000.0)
            for xin in (x + delta.float(), x):
                out[("fwd+1000", dtype)] = max(out.get(("fwd+1000", dtype), 0), y_bound(xin, gamma, beta, dtype)[2])
        for M, D in [(5, d) for d in BWD_D] + [(197, 260), (4103, 128), (4103, 772), (4103, 2048)]:
            for wd in (True, False):
                errs = _bwd_bounds(*_bwd_inputs(M, D, dtype, wd), dtype)[2]
                for k, v in errs.items():
                    key = ("bwd " + ("fwd-part" if k in ("x_out", "y") else "grads"), dtype)
                    out[key] = max(out.get(key, 0), v)
    return out
