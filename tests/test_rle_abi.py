"""The run-length encoding entry points (csrc/rle.hip: as_rle_count, as_rle_encode) without a GPU: exports, the workspace
size, the argument checks that return before any launch, and the rule that CPU tensors never reach the kernels."""
import ctypes

import numpy as np
import pytest
import torch

from attentionshift_amd import _lib, inference as I, ops

NAMES = ("as_rle_tile", "as_rle_workspace_bytes", "as_rle_count", "as_rle_encode")
FAKE = 4096                                       # a non-null, aligned address: every case below returns before a launch


def test_library_exports_the_rle_entry_points():
    from attentionshift_amd.csrc import build
    lib = ctypes.CDLL(build.build(verbose=False))
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name


def test_workspace_is_the_bases_and_the_cell_offsets_and_counts():
    lib = _lib.load()
    rows, cols = ops.rle_tile()
    assert 0 < rows <= 255 and cols > 0 and cols % 64 == 0            # a cell's count is one byte; whole lanes
    seg = lambda H: -(-H // rows)
    for n, H, W in ((1, 1, 1), (100, 1024, 1024), (7, 67, 131), (3, rows, 5), (3, rows + 1, 5), (65535, 1, 1)):
        assert lib.as_rle_workspace_bytes(n, H, W) == 8 * (n + 1) + 5 * n * seg(H) * W, (n, H, W)
    assert lib.as_rle_workspace_bytes(65535, 46340, 46340) == 8 * 65536 + 5 * 65535 * seg(46340) * 46340   # a size_t
    for n, H, W in ((0, 8, 8), (4, 0, 8), (4, 8, 0), (-1, 8, 8), (4, -8, 8)):
        assert lib.as_rle_workspace_bytes(n, H, W) == 0


def _count(lib, masks, n, H, W, totals=FAKE, ws=FAKE, ws_bytes=1 << 60):
    return lib.as_rle_count(masks, n, H, W, totals, ws, ws_bytes, None)


def _encode(lib, masks, n, H, W, totals=FAKE, ws=FAKE, ws_bytes=1 << 60, pos=FAKE, pos_cap=10, out=FAKE, out_cap=100, lens=FAKE):
    return lib.as_rle_encode(masks, n, H, W, totals, ws, ws_bytes, pos, pos_cap, out, out_cap, lens, None)


def test_bad_arguments_return_error_codes_without_launching():
    lib = _lib.load()
    for call in (_count, _encode):
        assert call(lib, None, 2, 8, 8) == -1                           # AS_E_BADARG: null pointers
        assert b"null" in lib.as_last_error()
        assert call(lib, FAKE, 2, 8, 8, totals=None) == -1
        assert call(lib, FAKE, 2, 8, 8, ws=None) == -1
        assert call(lib, FAKE, -1, 8, 8) == -1                          # negative sizes
        assert call(lib, FAKE, 2, -8, 8) == -1
        assert call(lib, FAKE, 2, 8, -8) == -1
        assert call(lib, FAKE, 2, 46341, 46341) == -2                   # AS_E_UNSUPPORTED: H * W = 2^31 + 88281 pixels
        assert call(lib, FAKE, 2, 1 << 16, 1 << 15) == -2               # H * W = 2^31
        assert call(lib, FAKE, 65536, 8, 8) == -2                       # n > 65535
        assert b"65535" in lib.as_last_error()
        assert call(lib, FAKE, 2, 8, 8, ws_bytes=lib.as_rle_workspace_bytes(2, 8, 8) - 1) == -4    # AS_E_WORKSPACE
        assert call(lib, FAKE, 2, 8, 8, ws=FAKE + 4) == -1              # alignment
        assert call(lib, None, 0, 8, 8, totals=None, ws=None, ws_bytes=0) == 0        # nothing to do
        assert call(lib, None, 3, 0, 8, totals=None, ws=None, ws_bytes=0) == 0
        assert call(lib, None, 3, 8, 0, totals=None, ws=None, ws_bytes=0) == 0
    assert _encode(lib, FAKE, 2, 8, 8, out=None) == -1
    assert _encode(lib, FAKE, 2, 8, 8, lens=None) == -1
    assert _encode(lib, FAKE, 2, 8, 8, pos=None) == -1                  # positions expected (capacity 10) but no buffer
    assert _encode(lib, FAKE, 2, 8, 8, lens=FAKE + 4) == -1
    assert lib.as_rle_tile(None, None) == -1


def test_wrapper_refuses_cpu_tensors_and_other_types():
    with pytest.raises(ops.AttnShiftError):
        ops.rle_encode(torch.zeros(2, 8, 8, dtype=torch.bool))
    with pytest.raises(ops.AttnShiftError):
        ops.rle_encode(torch.zeros(2, 8, 8, dtype=torch.uint8))


def test_cpu_inputs_never_reach_the_kernels(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device route was taken for a CPU input")
    monkeypatch.setattr(ops, "rle_encode", boom)
    m = np.zeros((2, 4, 6), bool)
    m[0, 1:3, 2:5] = True
    want = [{"size": [4, 6], "counts": b"9220003"}, {"size": [4, 6], "counts": b"h0"}]
    assert I.rle_encode(m) == want
    assert I.rle_encode(torch.from_numpy(m)) == want
    assert I.encode_mask_results([[m[0]], [m[1]]]) == [[want[0]], [want[1]]]
