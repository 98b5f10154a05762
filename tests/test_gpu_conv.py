"""as_conv2d_fwd (csrc/conv.hip through ops.conv2d_nhwc) against F.conv2d in fp64 on the CPU, applied to the bf16-rounded
operands.

The bar.  The kernel sums K = ksize^2 * Cin exact bf16 products, a bias and (with `add`) one more term in fp32, in its own
order: it lies within err(K, S) = (K + 3) * 2^-23 * S of the exact value, S = the same convolution of |x| and |w| plus |bias|
plus |add| in fp64 (one fp32 ulp of the running magnitude per accumulated term; ReLU is 1-Lipschitz).  A bf16 output adds
one rounding: 2^-8 * |y|.  x is uniform in [0.25, 1.25): a halo read from the wrong place, or a padding tap that is not
zero, moves the result by about a whole product -- thousands of bars.  The weights are normal / sqrt(K) times a factor that
differs for every (ky, kx) and drifts along ci and co, so that no swap of taps or channels goes unseen.
"""
import pytest
import torch
import torch.nn.functional as F

from attentionshift_amd import ops
from attentionshift_amd.neck import nearest_src_index

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23

#        name              B  H   W   Cin  Cout k  out              bias   act     add     strided  tile
CASES = [
    ("one_pixel",         (1, 1,  1,  32,  16,  3), torch.bfloat16, True,  "none", None,   False,   32),
    ("below_a_tile",      (2, 2,  3,  64,  16,  3), torch.bfloat16, False, "relu", None,   False,   32),
    ("odd_sizes",         (2, 9,  13, 96,  64,  3), torch.bfloat16, True,  "none", None,   False,   32),
    ("odd_sizes_nobias",  (2, 9,  13, 96,  64,  3), torch.float32,  False, "relu", None,   False,   32),
    ("odd_sizes_add",     (2, 9,  13, 96,  64,  1), torch.bfloat16, True,  "none", (4, 6), False,   32),
    ("shipped_channels",  (1, 37, 50, 256, 256, 3), torch.bfloat16, True,  "none", None,   False,   128),
    ("shipped_relu_f32",  (1, 37, 50, 256, 256, 3), torch.float32,  True,  "relu", None,   False,   128),
    ("lateral_strided",   (2, 18, 26, 768, 256, 1), torch.bfloat16, True,  "none", (9, 13), True,   128),
    ("lateral_nobias",    (2, 18, 26, 768, 256, 1), torch.bfloat16, False, "none", None,   True,    128),
    ("rpn_heads_f32",     (1, 20, 24, 256, 16,  1), torch.float32,  True,  "none", None,   False,   32),
]


def operands(shape, add_hw, seed):
    B, H, W, Cin, Cout, k = shape
    gen = torch.Generator().manual_seed(seed)
    x = (torch.rand(B, H, W, Cin, generator=gen) + 0.25).to(torch.bfloat16)
    K = k * k * Cin
    w = torch.randn(Cout, Cin, k, k, generator=gen) / K ** 0.5
    ky, kx = torch.arange(k).view(1, 1, k, 1), torch.arange(k).view(1, 1, 1, k)
    ci, co = torch.arange(Cin).view(1, Cin, 1, 1), torch.arange(Cout).view(Cout, 1, 1, 1)
    w = w * (1.0 + 0.5 * ky - 0.3 * kx + 0.25 * ci / Cin - 0.125 * co / Cout)
    w = w.to(torch.bfloat16)
    bias = torch.randn(Cout, generator=gen)
    add = None if add_hw is None else (torch.rand(B, add_hw[0], add_hw[1], Cout, generator=gen) * 2 - 0.5).to(torch.bfloat16)
    return x, w, bias, add


_REF = {}


def reference(shape, add_hw, seed):
    """-> (x, w_oihw, bias, add, y64 without bias / add / act, S without |bias| / |add|), computed once per shape"""
    key = (shape, add_hw)
    if key not in _REF:
        x, w, bias, add = operands(shape, add_hw, seed)
        k = shape[5]
        xd, wd = x.double().permute(0, 3, 1, 2), w.double()
        y = F.conv2d(xd, wd, None, padding=(k - 1) // 2).permute(0, 2, 3, 1)
        S = F.conv2d(xd.abs(), wd.abs(), None, padding=(k - 1) // 2).permute(0, 2, 3, 1)
        _REF[key] = (x, w, bias, add, y, S)
    return _REF[key]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_conv_lies_within_the_accumulation_bound(case):
    name, shape, out_dtype, with_bias, act, add_hw, strided, tile = case
    B, H, W, Cin, Cout, k = shape
    x, w, bias, add, y, S = reference(shape, add_hw, 100 + len(name))
    if with_bias:
        y, S = y + bias.double(), S + bias.double().abs()
    if add is not None:
        sy, sx = nearest_src_index(H, add_hw[0]), nearest_src_index(W, add_hw[1])
        up = add.double()[:, sy][:, :, sx]
        assert torch.equal(up.permute(0, 3, 1, 2), F.interpolate(add.double().permute(0, 3, 1, 2), size=(H, W), mode="nearest"))
        y, S = y + up, S + up.abs()
    if act == "relu":
        y = y.clamp(min=0)
    bar = (k * k * Cin + 3) * EPS * S + (2.0 ** -8 * y.abs() if out_dtype == torch.bfloat16 else 0.0)

    assert ops.conv2d_tile_n(Cout) == tile                              # which tile variant the launcher takes
    if strided:                                                          # a batch-strided view inside a token tensor
        buf = torch.full((B, H * W + 4, Cin), 100.0, dtype=torch.bfloat16, device="cuda")
        xd = buf[:, 1:1 + H * W].view(B, H, W, Cin)
        xd.copy_(x)
        assert xd.stride(0) == (H * W + 4) * Cin and xd.data_ptr() != buf.data_ptr()
    else:
        xd = x.cuda()
    wp = ops.pack_conv_weight(w.cuda())
    assert tuple(wp.shape) == (Cout, k, k, Cin)
    args = dict(bias=bias.cuda() if with_bias else None, ksize=k, act=act, add=None if add is None else add.cuda(),
                out_dtype=out_dtype)
    got = ops.conv2d_nhwc(xd, wp, **args)
    again = ops.conv2d_nhwc(xd, wp, **args)
    torch.cuda.synchronize()
    assert got.dtype == out_dtype and tuple(got.shape) == (B, H, W, Cout) and got.is_contiguous()
    assert torch.equal(got, again), "two calls on the same inputs differ"
    ratio = float(((got.cpu().double() - y).abs() / bar).max())
    print(f"CONV_RATIO {name} tile_n={tile} worst error / bar = {ratio:.4f}")
    assert bool(torch.isfinite(got).all()) and ratio <= 1.0, f"{name}: worst error is {ratio:.3f} bars"


def test_padding_taps_are_exact_zeros_whatever_lies_beside_the_image():
    """A one-row image between two rows of infinities in one buffer: the taps above and below the image must not be read
    into the sum (0 * inf would be NaN)."""
    B, H, W, Cin, Cout = 1, 1, 5, 32, 16
    buf = torch.full((3, W, Cin), float("inf"), dtype=torch.bfloat16, device="cuda")
    buf[1] = 0.5
    w = torch.ones(Cout, Cin, 3, 3)
    got = ops.conv2d_nhwc(buf[1:2].view(B, H, W, Cin), ops.pack_conv_weight(w.cuda()), ksize=3, out_dtype=torch.float32)
    want = torch.tensor([2.0, 3.0, 3.0, 3.0, 2.0]) * Cin * 0.5
    assert torch.equal(got.cpu()[0, 0], want[:, None].expand(W, Cout))


def test_wrapper_checks_shapes():
    x = torch.zeros(1, 4, 4, 32, dtype=torch.bfloat16, device="cuda")
    w = torch.zeros(16, 3, 3, 32, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ops.AttnShiftError):
        ops.conv2d_nhwc(x, w, ksize=1)
    with pytest.raises(ops.AttnShiftError):
        ops.conv2d_nhwc(x.float(), w)
    with pytest.raises(ops.AttnShiftError):
        ops.conv2d_nhwc(x, w, add=torch.zeros(1, 2, 2, 32, dtype=torch.bfloat16, device="cuda"))
    with pytest.raises(ops.AttnShiftError):
        ops.conv2d_nhwc(x, w, act="gelu")
    with pytest.raises(ops.AttnShiftError):                              # the kernel's contract: Cout % 16
        ops.conv2d_nhwc(x, torch.zeros(8, 3, 3, 32, dtype=torch.bfloat16, device="cuda"))
