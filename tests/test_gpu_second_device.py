"""The C library on a second GPU of the same process (csrc/launch.h: the dynamic-LDS opt-in, the CU count and the side
streams are kept per device).  The same seeded operands go through the C ABI on device 0 and then, under
torch.cuda.device(1), on device 1 -- raw pointers and that device's current stream, not `ops`, whose stream helper is
one-GPU-per-process by design.  Every call must return 0 on device 1 and give device 0's result.

  as_linear_fwd  bf16 2048 x 1024 x 128: 64 tiles of 256 x 128, the fewest the persistent ping-pong kernel takes (its 144 KiB
                 of LDS need the opt-in; whole tiles, no stream-K tail).  torch.equal: the kernel is bitwise reproducible
                 (test_gpu_gemm_pp.test_linear_equals_reference_and_gemm_hip_bitwise).
  as_sdpa_fwd    bf16 B = 1, h = 2, N = 300, as dispatched by default and with the last q-tile forced through the key-split
                 kernels on the side stream (AS_SDPA_TAIL=1, AS_SDPA_IMPL=3).  No existing test pins the forward bit for bit,
                 so the bound is the oracle test's (test_sdpa_bf16_deferred_max_and_spikes): max 2e-2 / mean 3e-3 of the
                 range, lse 1e-4 relative + 1e-3.
  as_sdpa_bwd    the same size, fed device 0's forward on both devices; dQ runs on the side stream.  torch.equal
                 (test_sdpa_bwd_full_size_properties asserts run-to-run bitwise equality)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

M, NOUT, K = 2048, 1024, 128
B, H, N = 1, 2, 300


def _inputs():
    from attentionshift_amd import ops
    g = torch.Generator().manual_seed(2048)
    x = torch.randn(M, K, generator=g).bfloat16()
    w = (torch.randn(NOUT, K, generator=g) * K ** -0.5).bfloat16()
    b = torch.randn(NOUT, generator=g)
    q, k, v = (torch.randn(B, H, N, 64, generator=g) for _ in range(3))
    npad = ops.npad(N)
    qp = torch.zeros(B, H, npad, 64, dtype=torch.bfloat16)
    kp = torch.zeros_like(qp)
    vtp = torch.zeros(B, H, 64, npad, dtype=torch.bfloat16)
    qp[:, :, :N], kp[:, :, :N], vtp[:, :, :, :N] = (q * ops.QSCALE).bfloat16(), k.bfloat16(), v.bfloat16().transpose(-1, -2)
    d_o = torch.randn(B, N, 64 * H, generator=g).bfloat16()
    return x, w, b, ops.q_to_fragment_major(qp), kp, vtp, d_o


def _run(lib, d, cpu, fwd=None):
    """the calls on device d -> (linear, o, lse, o_tail, lse_tail, dqkv) on the host; the backward takes `fwd` = (o, lse)"""
    import os
    with torch.cuda.device(d):
        dev = torch.device("cuda", d)
        x, w, b, qf, kp, vtp, d_o = (t.to(dev).contiguous() for t in cpu)
        st = torch.cuda.current_stream(d).cuda_stream
        out = torch.empty(M, NOUT, dtype=torch.bfloat16, device=dev)
        assert lib.as_linear_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), M, NOUT, K, 1, 0, st) == 0, d
        res = [out]
        for env in ({}, {"AS_SDPA_TAIL": "1", "AS_SDPA_IMPL": "3"}):            # (both read per call)
            os.environ.update(env)
            try:
                nb = lib.as_sdpa_fwd_workspace_bytes(B, N, H, 1)
                assert nb > 0 or not env, "the key-split tail needs its workspace"
                ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
                o = torch.empty(B, N, 64 * H, dtype=torch.bfloat16, device=dev)
                lse = torch.empty(B, H, N, dtype=torch.float32, device=dev)
                assert lib.as_sdpa_fwd(qf.data_ptr(), kp.data_ptr(), vtp.data_ptr(), o.data_ptr(), lse.data_ptr(), ws.data_ptr(), nb,
                                       B, N, H, 1, st) == 0, (d, env)
            finally:
                for name in env:
                    del os.environ[name]
            res += [o, lse]
        o, lse = (t.to(dev) for t in fwd) if fwd is not None else res[1:3]
        nb = lib.as_sdpa_bwd_workspace_bytes(B, N, H, 1)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        dqkv = torch.empty(B, N, 3 * 64 * H, dtype=torch.bfloat16, device=dev)
        assert lib.as_sdpa_bwd(qf.data_ptr(), kp.data_ptr(), vtp.data_ptr(), o.data_ptr(), d_o.data_ptr(), lse.data_ptr(), dqkv.data_ptr(),
                               ws.data_ptr(), nb, B, N, H, 1, st) == 0, d
        res.append(dqkv)
        torch.cuda.synchronize(d)
        return [t.cpu() for t in res]


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs in one process")
def test_second_device_gives_the_first_device_s_results():
    from attentionshift_amd import _lib
    lib = _lib.load()
    cpu = _inputs()
    first = _run(lib, 0, cpu)
    second = _run(lib, 1, cpu, fwd=first[1:3])
    assert torch.isfinite(first[0].float()).all() and torch.isfinite(first[5].float()).all()
    assert torch.equal(second[0], first[0]), "as_linear_fwd"
    for name, i in (("as_sdpa_fwd", 1), ("as_sdpa_fwd (key-split tail)", 3)):
        ref, got = first[i].double(), second[i].double()
        scale = ref.abs().max().item() + 1e-30
        err = (ref - got).abs()
        print(f"[second device] {name}: max {err.max().item() / scale:.3g} mean {err.mean().item() / scale:.3g} of the range")
        assert err.max().item() / scale < 2e-2 and err.mean().item() / scale < 3e-3, name
        assert torch.allclose(second[i + 1], first[i + 1], rtol=1e-4, atol=1e-3), name + " lse"
    assert torch.equal(second[5], first[5]), "as_sdpa_bwd"
