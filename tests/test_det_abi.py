"""The detection-candidate entry points (csrc/det.hip: as_det_candidates) without a GPU: exports, the workspace size, the
argument checks that return before any launch (a launch here, without a device, would return AS_E_LAUNCH = -3), and the rule
that CPU tensors never reach the kernels."""
import ctypes

import pytest
import torch

from attentionshift_amd import _lib, ops

FAKE = 4096                                       # a non-null, 16-byte aligned address: every case below returns before a launch


def test_library_exports_the_det_entry_points():
    from attentionshift_amd.csrc import build
    lib = ctypes.CDLL(build.build(verbose=False))
    for name in ("as_det_candidates", "as_det_candidates_workspace_bytes"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.load().as_version() == 100


def _r16(b):
    return (b + 15) // 16 * 16


def test_workspace_is_the_keys_the_row_offsets_and_the_probabilities():
    lib = _lib.load()
    for n, K in ((1, 1), (63, 5), (120, 5), (1000, 20), (1000, 80), (3300, 20), (65535, 16), (4112, 255)):
        cap = min(n * K, 65535)
        want = _r16(8 * cap) + _r16(4 * (n + 1)) + _r16(4 * n * (K + 1))
        assert lib.as_det_candidates_workspace_bytes(n, K) == want, (n, K)
        assert want == 16 * -(-cap // 2) + 16 * -(-(n + 1) // 4) + 16 * -(-n * (K + 1) // 4)     # as the header states it
    for n, K in ((0, 20), (100, 0), (-1, 20), (100, -5)):
        assert lib.as_det_candidates_workspace_bytes(n, K) == 0


def _call(lib, n=100, K=20, Kb=None, boxes=FAKE, deltas=FAKE, scores=FAKE, shape="make", scale=None, norm="make", prob=None,
          outs=FAKE, ws=FAKE, ws_bytes=1 << 60):
    sh = (ctypes.c_float * 2)(240, 320) if shape == "make" else shape
    ms = (ctypes.c_float * 8)(0, 0, 0, 0, 1, 1, 1, 1) if norm == "make" else norm
    out = [outs] * 6 if not isinstance(outs, list) else outs
    return lib.as_det_candidates(boxes, deltas, K if Kb is None else Kb, scores, 1, n, K, 0.05,
                                 ctypes.addressof(sh) if sh is not None else None, scale,
                                 ctypes.addressof(ms) if ms is not None else None, 4.135, prob, *out, ws, ws_bytes, None)


def test_bad_arguments_return_error_codes_without_launching():
    lib = _lib.load()
    assert _call(lib, boxes=None) == -1                                  # AS_E_BADARG: null pointers
    assert b"null" in lib.as_last_error()
    assert _call(lib, scores=None) == -1
    assert _call(lib, norm=None) == -1                                   # deltas need the means and stds
    assert _call(lib, ws=None) == -1
    for k in range(6):
        assert _call(lib, outs=[FAKE] * k + [None] + [FAKE] * (5 - k)) == -1
    assert _call(lib, n=-1) == -1                                        # below the minima
    assert _call(lib, K=0) == -1
    assert _call(lib, Kb=2) == -1                                        # Kb is 1 or K
    assert b"Kb = 2" in lib.as_last_error()
    assert _call(lib, Kb=0) == -1
    assert _call(lib, ws=FAKE + 8) == -1                                 # alignment
    assert _call(lib, outs=[FAKE + 4] + [FAKE] * 5) == -1
    assert _call(lib, outs=[FAKE, FAKE + 8] + [FAKE] * 4) == -1
    assert _call(lib, boxes=FAKE + 4) == -1
    need = lib.as_det_candidates_workspace_bytes(100, 20)
    assert _call(lib, ws_bytes=need - 1) == -4                           # AS_E_WORKSPACE
    assert _call(lib, ws_bytes=0, Kb=1) == -4
    assert _call(lib, n=0, boxes=None, deltas=None, scores=None, outs=None, ws=None, ws_bytes=0) == 0      # nothing to do


def test_problems_beyond_the_limits_are_unsupported_without_launching():
    lib = _lib.load()
    assert _call(lib, n=65536, K=1) == -2                                # AS_E_UNSUPPORTED
    assert b"65535" in lib.as_last_error()
    assert _call(lib, n=100, K=256) == -2
    assert _call(lib, n=4113, K=255) == -2                               # n * K > 2^20
    assert _call(lib, n=65535, K=17) == -2
    assert _call(lib, n=65535, K=16, ws_bytes=0) == -4                   # 2^20 - 16 fits: gets as far as the workspace
    assert _call(lib, n=4112, K=255, ws_bytes=0) == -4


def test_wrapper_refuses_cpu_tensors():
    with pytest.raises(ops.AttnShiftError):
        ops.det_candidates(torch.zeros(3, 4), torch.zeros(3, 8), torch.zeros(3, 3), 0.05, (32, 32, 3))
    with pytest.raises(ops.AttnShiftError):
        ops.det_candidates(torch.zeros(3, 8), None, torch.zeros(3, 3), 0.05, apply_softmax=False)
