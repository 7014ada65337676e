"""Results at source size (``results_at_source``), host side: the box rule ``fewshot_ds.boxes_to_source``
- exact, no tolerance anywhere - and the C-ABI surface of the two entry points behind the feature."""
import os
import re

import numpy as np
import pytest

from fgn_amd import fewshot_ds as fd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_boxes_to_source_known_answer():
    b = np.array([[20, 10, 40, 30]], np.float32)                    # YXYX in a (100, 200) network
    got = fd.boxes_to_source(b, (50, 400), (100, 200))              # s_y = 2, s_x = 0.5
    assert got.dtype == np.float32 and got.tolist() == [[10, 20, 20, 60]]
    assert fd.boxes_to_source(b, (50, 400), (100, 200), order='yxyx').tolist() == [[10, 20, 20, 60]]
    xyxy = np.ascontiguousarray(b[:, [1, 0, 3, 2]])
    got = fd.boxes_to_source(xyxy, (50, 400), (100, 200), order='xyxy')
    assert got.dtype == np.float32 and got.tolist() == [[20, 10, 60, 20]]
    assert b.tolist() == [[20, 10, 40, 30]]                          # the caller's array is never written


def test_boxes_to_source_properties():
    rng = np.random.RandomState(5)
    b = (rng.rand(257, 4) * 300 - 50).astype(np.float32)
    b[0] = [0, -0.0, 1e-30, 1e30]
    for (h, w), (H, W) in (((101, 77), (128, 128)), ((150, 131), (128, 128)), ((480, 640), (800, 1333)),
                           ((1, 200), (64, 96)), ((200, 1), (64, 96)), ((37, 53), (64, 96)), ((16384, 3), (7, 16384))):
        sy, sx = np.float32(H / h), np.float32(W / w)
        got = fd.boxes_to_source(b, (h, w), (H, W))
        assert got is not b and got.dtype == np.float32 and got.shape == b.shape
        for c, s in enumerate((sy, sx, sy, sx)):
            want = np.float32(b[:, c]) / np.float32(s)               # correctly rounded f32 division, once
            assert want.dtype == np.float32 and got[:, c].tobytes() == want.tobytes(), ((h, w), c)
        got = fd.boxes_to_source(b, (h, w), (H, W), order='xyxy')
        for c, s in enumerate((sx, sy, sx, sy)):
            assert got[:, c].tobytes() == (b[:, c] / s).tobytes(), ((h, w), c)
        # ... which is the float64 quotient rounded to f32 (53 >= 2 * 24 + 2 bits: the double rounding is innocuous for
        # a division of normal numbers)
        assert np.array_equal(fd.boxes_to_source(b[1:], (h, w), (H, W))[:, 0],
                              (b[1:, 0].astype(np.float64) / np.float64(sy)).astype(np.float32))
    # equal size: the same object, like resize_query
    assert fd.boxes_to_source(b, (128, 96), (128, 96)) is b
    assert fd.boxes_to_source(b, (128, 96), (128, 96), order='xyxy') is b
    empty = np.zeros((0, 4), np.float32)
    assert fd.boxes_to_source(empty, (5, 7), (10, 10)).shape == (0, 4)
    for bad in (b.astype(np.float64), b[:, :3], b[0], b.tolist()):
        with pytest.raises(ValueError):
            fd.boxes_to_source(bad, (5, 7), (10, 10))
    with pytest.raises(ValueError):
        fd.boxes_to_source(b, (5, 7), (10, 10), order='xywh')
    with pytest.raises(ValueError):
        fd.boxes_to_source(b, (0, 7), (10, 10))
    with pytest.raises(ValueError):
        fd.boxes_to_source(b, (5, 7), (10, fd.RESIZE_MAX_DIM + 1))


def test_abi_33_declares_and_binds_the_source_size_entry_points():
    from fgn_amd import lib
    header = open(os.path.join(ROOT, 'include', 'fgn_hip.h')).read()
    declared = set(re.findall(r'\b(fgn_[a-z0-9_]+)\s*\(', header))
    for name in ('fgn_mask_rle_src', 'fgn_mask_overlap_src_i32'):
        assert name in declared and name in lib.SIGNATURES
        # one ctypes argument per declared parameter
        params = re.search(r'\b' + name + r'\s*\(([^)]*)\)', header).group(1)
        assert len(lib.SIGNATURES[name][1]) == len(params.split(','))
    assert lib.ABI_VERSION == 33


def test_the_flag_needs_qry_resize_to_on_every_entry():
    """``results_at_source`` without ``qry_resize_to`` is a contract error raised on the host, before the GPU is asked
    for (this test has none); ``forward_train`` does not take the flag."""
    import inspect
    import torch
    from fgn_amd.config import tiny_config
    from fgn_amd.detector import FGN
    cfg = tiny_config(1, 1, 2)
    m = FGN(1, 1, backbone=cfg['backbone'], rpn_head=cfg['rpn_head'], roi_head=cfg['roi_head'])
    img = torch.zeros((1, 3, 64, 64))
    with pytest.raises(ValueError, match='qry_resize_to'):
        m.simple_test(img, results_at_source=True, rescale=True)
    with pytest.raises(ValueError, match='qry_resize_to'):
        m.detect_device(img, None, None, None, None, results_at_source=True)
    for fn in (FGN.simple_test, FGN.detect_device, FGN.pack_results):
        p = inspect.signature(fn).parameters['results_at_source']
        assert p.default is False
    assert 'results_at_source' not in inspect.signature(FGN.forward_train).parameters
    assert 'rescale' in inspect.signature(FGN.simple_test).parameters
