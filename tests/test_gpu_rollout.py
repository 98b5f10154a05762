"""A3 on the kernel that actually runs on the BASELINE ViT configurations, and on every other kernel `as_rollout_step` can pick.

`as_rollout_step` takes `rollout_step4_kernel` for bf16 tensors with h % 4 == 0 and a workspace (csrc/rollout.hip) --
every ViT-B (h = 12) and ViT-L (h = 16) step.  The first three tests hold THAT kernel, in both its forms (all T point-token
rows; the <= 32-row form behind `rows=`), to the oracle's `attns_project_to_feature` restatement (stdroi:1257-1272 + the row
slice of :2272): the oracle builds the dense head-mean attention of every layer from the same bf16-rounded operands and
multiplies the augmented matrices; the device recomputes attention tiles from (q, k, lse).  bf16 tolerance as the
existing 3-head test (3e-2 of the range; observed ~1e-2: q/k are bf16, the roll-out operand R is carried in bf16).

The tests below them walk the whole dispatch of `launch_rollout_step2` (`expected_kernel` restates it; `test_chain_cases_
reach_every_kernel` fails when a later dispatch change orphans a path) at the geometry edges of the 32-row R blocks, the
32- / 128-column blocks and Npad = round_up(N, 64), against an fp64 reference of the same operands, with and without a
workspace, with NaN in every padded row / column of q, k and v^T, and -- one step at a time -- on a SIGNED random R
(`step_ref`), where a dropped contraction block cannot hide behind the row normalisation.  The f32-h16 cases (the ViT-L
parity path) are the ones that found a bug: `as_rollout_step` used to reject them ("LDS 172032 B exceeds 160 KiB"); they now
run rollout_step2_kernel<float, 4> with a single exchange slab.
"""
import ctypes
import functools

import pytest
import torch

import attnshift_oracle as O

gpu = pytest.mark.gpu            # (not a module-wide pytestmark: test_step_ref_chain_equals_the_oracle_rollout runs on the host)
torch.set_grad_enabled(False)

BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def ops():
    from attentionshift_amd import ops as _ops
    _ops._lib.load()
    return _ops


def dev(x):
    return x.cuda().contiguous()


def rel_to_range(ref, got):
    ref, got = ref.double().cpu(), got.double().cpu()
    scale = ref.abs().max().item() + 1e-30
    err = (ref - got).abs()
    return err.max().item() / scale, err.mean().item() / scale


def _layers(ops, B, N, h, L, seed, scale=3.0):
    """L attention layers on seeded inputs: device states (q, k, lse) and the oracle's head-mean matrices [B,N,N] of the
    same bf16-rounded operands."""
    D = 64 * h
    states, means = [], []
    for l in range(L):
        g = torch.Generator().manual_seed(seed + l)
        x = torch.randn(B, N, D, generator=g).bfloat16()
        wqkv = (torch.randn(3 * D, D, generator=g) * (scale / D ** 0.5)).bfloat16()
        bqkv = torch.randn(3 * D, generator=g) * 0.1
        wproj = (torch.randn(D, D, generator=g) / D ** 0.5).bfloat16()
        bproj = torch.zeros(D)
        means.append(O.attention_head_mean(x.float(), wqkv.float(), bqkv, h))
        _, st = ops.attention_fwd(dev(x), dev(wqkv), dev(bqkv), dev(wproj), dev(bproj), h)
        states.append(st)
    return states, means


def _uses_step4(ops, st, T):
    """the dispatch condition of as_rollout_step (csrc/rollout.hip): bf16, h % 4 == 0, workspace supplied"""
    return st.q.dtype == torch.bfloat16 and st.h % 4 == 0 and ops._lib.load().as_rollout_step_workspace_bytes(st.B, st.N, T) > 0


@gpu
@pytest.mark.parametrize("B,N,h,T,L", [(2, 457, 4, 40, 4), (1, 1090, 12, 100, 3), (1, 300, 16, 100, 3)])
def test_rollout_step4_all_rows_match_oracle(ops, B, N, h, T, L):
    """full-T form (rollout_step4_kernel<4>): every point-token row of every partial product."""
    states, means = _layers(ops, B, N, h, L, 700 + N)
    assert _uses_step4(ops, states[0], T)
    ref = O.rollout_rows(means, T)
    got = ops.rollout_rows(states, T)
    assert got.shape == ref.shape
    mx, mean = rel_to_range(ref, got)
    assert mx < 3e-2 and mean < 2e-3, (mx, mean)
    # the rows are probability distributions over the tokens (row-stochastic factors): a dropped partial product or a
    # mis-weighted head group shows up here independently of the element-wise tolerance
    s = got.sum(-1)
    assert (s - 1).abs().max().item() < 2e-2, (s.min().item(), s.max().item())


@gpu
@pytest.mark.parametrize("B,N,h,T,L", [(2, 457, 4, 40, 4), (1, 1090, 12, 100, 3)])
def test_rollout_step4_row_subset_matches_oracle(ops, B, N, h, T, L):
    """<= 32-row form (rollout_step4_kernel<1> behind `rows=`, the form the RoI head uses for the matched tokens):
    against the SAME rows of the oracle's roll-out, not against the device's own full roll-out."""
    states, means = _layers(ops, B, N, h, L, 900 + N)
    ref = O.rollout_rows(means, T)                                        # [B, L, T, N]
    sel = torch.stack([torch.randperm(T, generator=torch.Generator().manual_seed(b))[:7] for b in range(B)])
    got = ops.rollout_rows(states, T, rows=dev(sel))
    want = torch.gather(ref, 2, sel[:, None, :, None].expand(-1, L, -1, N))
    assert got.shape == want.shape
    mx, mean = rel_to_range(want, got)
    assert mx < 3e-2 and mean < 2e-3, (mx, mean)


@gpu
def test_rollout_step4_config2_size_matched_rows_match_oracle(ops):
    """BASELINE config-2 token count (N = 4197, 12 heads), 3 layers, the first three point tokens matched (the rows the
    RoI head reads at G = 3): the device's recomputed-tile roll-out against the oracle's DENSE head-mean product
    (12 x 4197^2 softmax per layer on the host).  This is the launch geometry of the bench step: 33 column blocks x 5 head
    groups x 3 contraction splits, ragged last block (4197 = 131 * 32 + 5)."""
    B, N, h, T, L = 1, 4197, 12, 100, 3
    states, means = _layers(ops, B, N, h, L, 4197)
    sel = torch.tensor([[0, 1, 2]])
    got = ops.rollout_rows(states, T, rows=dev(sel)).cpu()                # [1, L, 3, N]
    # oracle, row-sliced by hand so the [N,N] products are [3,N] x [N,N] (stdroi:1257-1272 on rows N-T+{0,1,2})
    eye = torch.eye(N)
    run, outs = None, []
    for l in range(L - 1, -1, -1):
        aug = means[l][0] + eye
        aug = aug / aug.sum(-1, keepdim=True)
        run = aug[N - T + sel[0]] if run is None else run @ aug
        outs.append(run)
    want = torch.stack(outs)[None]
    mx, mean = rel_to_range(want, got)
    assert mx < 3e-2 and mean < 2e-3, (mx, mean)
    # what the consumer reads: columns [1:-T] as 64x64 CAMs; compare after its own min-max normalisation too
    cam_w = O.minmax_maps(want[0, :, :, 1:-T].reshape(-1, 64, 64))
    cam_g = O.minmax_maps(got[0, :, :, 1:-T].reshape(-1, 64, 64))
    assert (cam_w - cam_g).abs().max().item() < 5e-2


# ------------------------------------------------------------------------------------------------
# every kernel of launch_rollout_step2, at the geometry edges
# ------------------------------------------------------------------------------------------------
def step_ref(R_in, Pbar):
    """one roll-out step in fp64: R_out = R_in . (Pbar + I) / 2 (the augmented matrix's rows sum to 2)"""
    R_in, Pbar = R_in.double(), Pbar.double()
    return 0.5 * (R_in @ Pbar + R_in)


def test_step_ref_chain_equals_the_oracle_rollout():
    """The single-step reference of this file, chained from the top layer's rows, IS the oracle's roll-out (fp64, 1e-12):
    proves the tests' own reference without a device."""
    g = torch.Generator().manual_seed(5)
    B, N, T, L = 2, 50, 7, 4
    means = [torch.softmax(torch.randn(B, N, N, generator=g, dtype=torch.float64) * 2, dim=-1) for _ in range(L)]
    want = O.rollout_rows(means, T)                                      # [B, L, T, N]
    run = 0.5 * (means[-1] + torch.eye(N, dtype=torch.float64))[:, N - T:]
    got = [run]
    for l in range(L - 2, -1, -1):
        run = step_ref(run, means[l])
        got.append(run)
    got = torch.stack(got, dim=1)
    assert got.shape == want.shape
    assert (got - want).abs().max().item() < 1e-12


def rollout_nsplit(B, N):
    """csrc/rollout.hip rollout_nsplit: contraction split of the step2 / step3 kernels when a workspace is given"""
    wgs = -(-N // 32) * B
    ns = 1
    while ns < 16 and wgs * ns < 2048:
        ns *= 2
    return 1 if wgs >= 2048 else ns


def expected_kernel(dtype, h, use_workspace, T, B=1, N=297):
    """The dispatch of as_rollout_step / launch_rollout_step2 (csrc/rollout.hip), restated: (kernel, contraction split?)."""
    bf16 = dtype == BF16
    if bf16 and h % 4 == 0 and use_workspace:
        return ("rollout_step4_kernel<4>" if T > 32 else "rollout_step4_kernel<1>"), True
    split = use_workspace and rollout_nsplit(B, N) > 1
    if bf16 and h >= 8:
        return "rollout_step3_kernel", split
    return "rollout_step2_kernel<%s,%d>" % ("bf16" if bf16 else "float", -(-h // 4)), split


# (dtype, h, use_workspace, B, N, T).  First the dispatch list at one geometry (N = 297: ten contraction blocks, the last
# ragged; T = 97: four R blocks, the last with one live row) ...
CHAIN_CASES = [(F32, h, ws, 3 if h <= 6 else 1, 297, 97) for h in (1, 3, 6, 12, 16) for ws in (True, False)]
CHAIN_CASES += [(BF16, h, ws, 3, 297, 97) for h in (3, 5, 6) for ws in (True, False)]
CHAIN_CASES += [(BF16, 8, False, 1, 297, 97), (BF16, 12, False, 1, 297, 97), (BF16, 10, True, 1, 297, 97)]
CHAIN_CASES += [(BF16, h, True, 3 if h == 4 else 1, 297, 97) for h in (4, 8, 16)]
# ... then the geometry edges on an fp32 path, on step4 (<4> where T > 32, <1> below) and on step3:
#   (100, 100) row0 = 0, N < 128            (100, 1) a single row                  (129, 33) one live column in the second
#   (160, 32) N % 32 == 0, Npad = 192, exactly one R block      (192, 64) N == Npad        128-column block, T one past a block
#   (297, 128) T at its limit               (297, 97) above
GEOMS = [(100, 100), (100, 1), (129, 33), (160, 32), (192, 64), (297, 128)]
for _N, _T in GEOMS:
    CHAIN_CASES += [(F32, 3, True, 3, _N, _T), (F32, 6, False, 1, _N, _T), (BF16, 4, True, 3, _N, _T),
                    (BF16, 8, False, 1, _N, _T), (BF16, 10, True, 1, _N, _T)]
CHAIN_CASES += [(BF16, 12, True, 1, 100, 1), (BF16, 3, True, 1, 129, 33), (BF16, 6, False, 1, 160, 32)]


def _case_id(c):
    dtype, h, ws, B, N, T = c
    return "%s-h%d-%s-B%d-N%d-T%d" % ("bf16" if dtype == BF16 else "f32", h, "ws" if ws else "nows", B, N, T)


def test_chain_cases_reach_every_kernel():
    """The parameter list above reaches every kernel `launch_rollout_step2` can launch, and every kernel that has an
    unsplit form both split and unsplit; every geometry reaches an fp32 kernel, step4 and step3."""
    reached = {expected_kernel(d, h, ws, T, B, N) for d, h, ws, B, N, T in CHAIN_CASES}
    names = {k for k, _ in reached}
    want = {"rollout_step4_kernel<4>", "rollout_step4_kernel<1>", "rollout_step3_kernel", "rollout_step2_kernel<bf16,1>",
            "rollout_step2_kernel<bf16,2>"} | {"rollout_step2_kernel<float,%d>" % v for v in (1, 2, 3, 4)}
    assert names == want, (sorted(want - names), sorted(names - want))
    for k in want:
        if "step4" not in k:
            assert (k, True) in reached and (k, False) in reached, k
    assert len(set(CHAIN_CASES)) == len(CHAIN_CASES)
    for N, T in GEOMS + [(297, 97)]:
        ks = {expected_kernel(d, h, ws, T, B, N)[0] for d, h, ws, B, n, t in CHAIN_CASES if (n, t) == (N, T)}
        assert any("float" in k for k in ks) and "rollout_step3_kernel" in ks, (N, T, ks)
        assert ("rollout_step4_kernel<4>" if T > 32 else "rollout_step4_kernel<1>") in ks, (N, T, ks)


@functools.lru_cache(maxsize=None)
def _chain_layers(dtype, B, N, h, L=3):
    """L layers of seeded inputs -> (device states, fp64 head-mean matrices of the operands the device sees: the bf16-
    rounded x and W for bf16 cases).  Cached: a (dtype, B, N, h) serves every T, workspace mode and test that asks for it."""
    from attentionshift_amd import ops
    D = 64 * h
    states, means = [], []
    for l in range(L):
        g = torch.Generator().manual_seed(1000 * h + N + l)
        x = torch.randn(B, N, D, generator=g).to(dtype)
        wqkv = (torch.randn(3 * D, D, generator=g) * (3.0 / D ** 0.5)).to(dtype)
        bqkv = torch.randn(3 * D, generator=g) * 0.1
        wproj = (torch.randn(D, D, generator=g) / D ** 0.5).to(dtype)
        means.append(O.attention_head_mean(x.double(), wqkv.double(), bqkv.double(), h))
        _, st = ops.attention_fwd(dev(x), dev(wqkv), dev(bqkv), dev(wproj), dev(torch.zeros(D)), h)
        states.append(st)
    return tuple(states), tuple(means)


def _poisoned(ops, st):
    """the same layer state with NaN in every padded row of q and k and every padded column of v^T"""
    N = st.N
    q = ops.q_from_fragment_major(st.q.clone())
    q[:, :, N:] = float("nan")
    k, vt = st.k.clone(), st.vt.clone()
    k[:, :, N:] = float("nan")
    vt[..., N:] = float("nan")
    return ops.AttnLayerState(ops.q_to_fragment_major(q), k, vt, st.lse, st.B, st.N, st.h, st.dtype)


def _tols(dtype):
    """(max, mean) error of the range and the row-sum bound: the project's own (module docstring, test_gpu_kernels.py)"""
    return (3e-2, 2e-3, 2e-2) if dtype == BF16 else (1e-3, 1e-3, 1e-4)


@gpu
@pytest.mark.parametrize("case", CHAIN_CASES, ids=_case_id)
def test_rollout_chain_matches_fp64(ops, case):
    """Three layers (so every step kernel reads an `rf` a kernel wrote, writes one, and runs once with rf_out = NULL)
    against the fp64 roll-out of the fp64 head means; rows sum to 1.  Where N < Npad the same call on states whose padding
    is NaN must give the same bits: rollout_step4 DMAs whole padded Q blocks and has to DROP them (a select), not scale them."""
    dtype, h, ws, B, N, T = case
    states, means = _chain_layers(dtype, B, N, h)
    ref = O.rollout_rows(list(means), T)
    got = ops.rollout_rows(list(states), T, use_workspace=ws)
    assert got.shape == ref.shape == (B, 3, T, N)
    tmx, tmean, tsum = _tols(dtype)
    mx, mean = rel_to_range(ref, got)
    s = got.sum(-1)
    print("chain", _case_id(case), expected_kernel(dtype, h, ws, T, B, N), "max %.3g mean %.3g rowsum %.3g" %
          (mx, mean, (s - 1).abs().max().item()))
    assert torch.isfinite(got).all()
    assert mx < tmx and mean < tmean, (mx, mean)
    assert (s - 1).abs().max().item() < tsum, (s.min().item(), s.max().item())
    if N < ops.npad(N):
        again = ops.rollout_rows([_poisoned(ops, st) for st in states], T, use_workspace=ws)
        assert torch.isfinite(again).all()
        assert torch.equal(again, got), float((again - got).abs().max())
    else:
        assert (N, T) == (192, 64)


@gpu
@pytest.mark.parametrize("G", [1, 32, 33])
@pytest.mark.parametrize("dtype,h,ws", [(BF16, 4, True), (BF16, 8, False), (F32, 3, True)], ids=["step4", "step3", "f32"])
def test_rollout_row_subset_matches_fp64(ops, dtype, h, ws, G):
    """`rows=`: G selected rows (as_rollout_pack builds the operand) against the same rows of the fp64 roll-out; G = 33 moves
    the step4 case from the 32-row form <1> to <4>."""
    B, N, T = 2, 297, 97
    states, means = _chain_layers(dtype, B, N, h)
    kern = expected_kernel(dtype, h, ws, G, B, N)[0]
    if dtype == BF16 and h == 4:
        assert kern == ("rollout_step4_kernel<1>" if G <= 32 else "rollout_step4_kernel<4>")
    else:
        assert kern == ("rollout_step3_kernel" if dtype == BF16 else "rollout_step2_kernel<float,1>")
    ref = O.rollout_rows(list(means), T)
    sel = torch.stack([torch.randperm(T, generator=torch.Generator().manual_seed(10 * G + b))[:G] for b in range(B)])
    got = ops.rollout_rows(list(states), T, rows=dev(sel), use_workspace=ws)
    want = torch.gather(ref, 2, sel[:, None, :, None].expand(-1, 3, -1, N))
    assert got.shape == want.shape
    tmx, tmean, tsum = _tols(dtype)
    mx, mean = rel_to_range(want, got)
    s = got.sum(-1)
    print("subset", dtype, h, ws, G, "max %.3g mean %.3g rowsum %.3g" % (mx, mean, (s - 1).abs().max().item()))
    assert mx < tmx and mean < tmean, (mx, mean)
    assert (s - 1).abs().max().item() < tsum


# ------------------------------------------------------------------------------------------------
# one step at a time, through the C ABI, on a signed R
# ------------------------------------------------------------------------------------------------
def rf_slots(B, nkb, T, cols):
    """csrc/rollout.hip rf_slot: element index of R[b][i][k] in the fragment-major copy, for b < B, i < T, k in `cols`
    -> long [B, T, len(cols)]"""
    b = torch.arange(B)[:, None, None]
    i = torch.arange(T)[None, :, None]
    k = torch.as_tensor(cols)[None, None, :]
    rem = k & 31
    s2, r16 = rem >> 4, rem & 15
    lane = (i & 31) + 32 * ((r16 & 7) >> 2)
    t = (r16 >> 3) * 4 + (r16 & 3)
    return ((((b * nkb + (k >> 5)) * 4 + (i >> 5)) * 2 + s2) * 64 + lane) * 8 + t


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _one_step(ops, st, R, rf, T, use_ws, want_rf=True):
    """as_rollout_step on (R, rf) -> (R_out, rf_out)"""
    lib = ops._lib.load()
    dt = ops._dt(st.q)
    wbytes = lib.as_rollout_step_workspace_bytes(st.B, st.N, T) if use_ws else 0
    wsb = torch.empty(wbytes, device="cuda", dtype=torch.uint8) if wbytes else None
    R_out = torch.empty_like(R)
    rf_out = torch.empty_like(rf) if want_rf else None
    ops._lib.check(lib.as_rollout_step(_p(st.q), _p(st.k), _p(st.lse), _p(R), _p(rf), _p(R_out), _p(rf_out), _p(wsb), wbytes,
                                       st.B, st.N, st.h, T, dt, ops._stream()), "as_rollout_step")
    return R_out, rf_out


STEP_CASES = [(F32, 3, True, 97), (F32, 6, False, 97), (F32, 12, True, 97), (F32, 16, False, 97), (BF16, 3, True, 97),
              (BF16, 6, False, 97), (BF16, 8, False, 97), (BF16, 10, True, 97), (BF16, 4, True, 97), (BF16, 4, True, 20)]


def test_step_cases_reach_every_kernel():
    names = {expected_kernel(d, h, ws, T)[0] for d, h, ws, T in STEP_CASES}
    assert len(names) == 9 and names == {expected_kernel(d, h, ws, T, B, N)[0] for d, h, ws, B, N, T in CHAIN_CASES}


@gpu
@pytest.mark.parametrize("dtype,h,ws,T", STEP_CASES,
                         ids=["%s-h%d-%s-T%d" % ("bf16" if d == BF16 else "f32", h, "ws" if w else "nows", T) for d, h, w, T in STEP_CASES])
def test_rollout_single_step_on_a_signed_matrix(ops, dtype, h, ws, T):
    """as_rollout_pack + as_rollout_step on R_in ~ randn[T, N] (not a probability matrix: nothing normalises a missing block
    away) against step_ref in fp64; for bf16 the product term takes R_in rounded to bf16, the `rf` operand's dtype.  The
    fragment-major copy is checked slot by slot (rf_slots restates the layout), the slots of the padded contraction columns
    [N, 32 * ceil(N / 32)) are then filled with a finite 77: every kernel drops those contraction rows by itself (`live ?`
    in step2 / step3, the ragged-block select in step4).  The returned rf_out is checked the same way and fed to a second
    step.  Bounds: the chain tests' own, of the range of step_ref's output."""
    B, N = 2, 297
    states, means = _chain_layers(dtype, B, N, h)
    lib = ops._lib.load()
    dt = ops._dt(states[0].q)
    nkb = -(-N // 32)
    g = torch.Generator().manual_seed(31 * h + T)
    R = torch.randn(B, T, N, generator=g)
    Rd = dev(R)
    rf = torch.empty(lib.as_rollout_rfrag_bytes(B, N, dt) // (2 if dtype == BF16 else 4), device="cuda", dtype=dtype)
    ops._lib.check(lib.as_rollout_pack(_p(Rd), _p(rf), B, N, T, dt, ops._stream()), "as_rollout_pack")
    live, pad = rf_slots(B, nkb, T, list(range(N))), rf_slots(B, nkb, T, list(range(N, nkb * 32)))
    assert int(max(live.max(), pad.max())) < rf.numel()
    host = rf.cpu()
    assert torch.equal(host[live], R.to(dtype)) and (host[pad] == 0).all()
    host[pad] = 77.0
    rf = dev(host)
    tmx, tmean, _ = _tols(dtype)
    Rq = R.to(dtype).double()                                            # what the MFMA multiplies
    for n, st_i in enumerate((0, 1)):
        R_out, rf_out = _one_step(ops, states[st_i], Rd, rf, T, ws, want_rf=(n == 0))
        want = 0.5 * (Rq @ means[st_i] + R.double())
        mx, mean = rel_to_range(want, R_out)
        print("step", dtype, h, ws, T, n, expected_kernel(dtype, h, ws, T, B, N), "max %.3g mean %.3g" % (mx, mean))
        assert torch.isfinite(R_out).all()
        assert mx < tmx and mean < tmean, (n, mx, mean)
        if n == 0:                                                       # second step: from what the first one returned
            host = rf_out.cpu()
            assert torch.equal(host[live], R_out.cpu().to(dtype)) and (host[pad] == 0).all()
            R, Rd, rf = R_out.cpu(), R_out, rf_out
            Rq = R.to(dtype).double()


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("h", [3, 12])
def test_attn_mean_rows_on_unaligned_slices(ops, dtype, h):
    """as_attn_mean_rows with row ranges that start and end inside a 32-row tile, and the single last row, vs the fp64 head
    mean; every row is a distribution."""
    B, N = 2, 297
    states, means = _chain_layers(dtype, B, N, h)
    tmx, _, tsum = _tols(dtype)
    for row0, nrows in ((5, 70), (N - 1, 1), (31, 34)):
        got = ops.attn_mean_rows(states[0], row0, nrows)
        assert got.shape == (B, nrows, N)
        mx, mean = rel_to_range(means[0][:, row0:row0 + nrows], got)
        s = got.sum(-1)
        print("mean_rows", dtype, h, row0, nrows, "max %.3g mean %.3g rowsum %.3g" % (mx, mean, (s - 1).abs().max().item()))
        assert mx < tmx, (row0, nrows, mx)
        assert (s - 1).abs().max().item() < tsum, (row0, nrows)
