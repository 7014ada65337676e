"""uint8 image input, host side (no GPU): the normalisation table is the data loader's arithmetic bit for bit, the
``raw_uint8`` dataset form carries the same pixels, and the contract errors."""
import numpy as np
import pytest
import torch

from fgn_amd import ops
from fgn_amd.fewshot_ds import ClutteredCharsFewShotISEG
from fgn_amd.lib import FgnHipError

bits = lambda a: np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


@pytest.mark.parametrize('dataset', sorted(ClutteredCharsFewShotISEG.PARAMS))
def test_input_lut_is_the_loaders_arithmetic_bit_for_bit(dataset):
    par = ClutteredCharsFewShotISEG.PARAMS[dataset]
    mean, std = np.asarray(par['mean'], np.float32), np.asarray(par['std'], np.float32)
    lut = ops.input_lut(par['mean'], par['std'])
    assert lut.shape == (3, 256) and lut.dtype == np.float32 and lut.flags['C_CONTIGUOUS']
    # every byte value in every channel, as an [256,1,3] image through the loader's expression (fewshot_ds._norm)
    img = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, 2)
    want_np = ((img.astype(np.float32) / 255.0 - mean) / std).transpose(2, 0, 1).copy()[:, :, 0]
    assert np.array_equal(bits(lut), bits(want_np))
    # ToTensor + Normalize as torch spells them
    t = torch.from_numpy(img).float().div(255).sub(torch.from_numpy(mean)).div(torch.from_numpy(std))
    assert np.array_equal(bits(lut), bits(t[:, 0, :].t().contiguous().numpy()))
    assert np.isfinite(lut).all() and len(np.unique(bits(lut[0]))) == 256


@pytest.mark.parametrize('dataset', sorted(ClutteredCharsFewShotISEG.PARAMS))
def test_raw_uint8_samples_map_onto_the_float_samples(dataset):
    kw = dict(dataset=dataset, n_ways=3, k_shots=2, n_imgs=6, img_size=96, spp_img_size=48, seed=7)
    f32, u8 = ClutteredCharsFewShotISEG(**kw), ClutteredCharsFewShotISEG(**kw, raw_uint8=True)
    norm = u8.input_norm
    assert set(norm) == {'mean', 'std'}
    lut = ops.input_lut(**norm)
    ch = np.arange(3)
    for idx in (0, 3, 5):
        a, b = f32[idx], u8[idx]
        assert list(a) == list(b)
        assert b['qry_img'].dtype == torch.uint8 and tuple(b['qry_img'].shape) == (96, 96, 3)
        assert b['spp_imgs'].dtype == torch.uint8 and tuple(b['spp_imgs'].shape) == (6, 48, 48, 3)
        assert b['qry_img'].is_contiguous() and b['spp_imgs'].is_contiguous()
        q = lut[ch, b['qry_img'].numpy()].transpose(2, 0, 1)                     # [H,W,3] -> [3,H,W]
        s = lut[ch, b['spp_imgs'].numpy()].transpose(0, 3, 1, 2)
        assert np.array_equal(bits(q), bits(a['qry_img'].numpy()))
        assert np.array_equal(bits(s), bits(a['spp_imgs'].numpy()))
        for k in a:
            if k in ('qry_img', 'spp_imgs'):
                continue
            x, y = np.asarray(a[k]), np.asarray(b[k])
            assert x.dtype == y.dtype and np.array_equal(x, y), k


def test_u8hwc3_to_nhwc4_has_no_cpu_fallback():
    x = torch.zeros((1, 2, 2, 3), dtype=torch.uint8)
    lut = torch.zeros((3, 256))
    with pytest.raises(FgnHipError):
        ops.u8hwc3_to_nhwc4(x, lut)


def test_set_input_norm_contract():
    from fgn_amd.config import tiny_config
    from fgn_amd.detector import FGN
    from fgn_amd.weights import init_state_dict
    cfg = tiny_config(3, 2, width_div=2)
    model = FGN(3, 2, backbone=cfg['backbone'], rpn_head=cfg['rpn_head'], roi_head=cfg['roi_head'],
                test_cfg=cfg['test_cfg'], state_dict=init_state_dict(cfg, 0))
    assert model.input_lut is None
    for bad in (np.zeros((256, 3), np.float32), np.zeros((3, 255), np.float32), np.zeros(768, np.float32)):
        with pytest.raises(ValueError):
            model.set_input_norm(lut=bad)
    assert model.input_lut is None
    par = ClutteredCharsFewShotISEG.PARAMS['MNISTISEG']
    model._graphs['stale'] = object()
    model.set_input_norm(mean=par['mean'], std=par['std'])
    assert model._graphs == {}
    assert np.array_equal(bits(model.input_lut), bits(ops.input_lut(par['mean'], par['std'])))
    # with a table, a uint8 tensor is judged by its own layout; a float one goes the NCHW way
    assert model._image_dims(torch.zeros((2, 5, 7, 3), dtype=torch.uint8), 'qry_img') == ((2,), 5, 7)
    assert model._image_dims(torch.zeros((2, 3, 5, 7)), 'qry_img') == ((2,), 5, 7)
    assert model._image_dims(torch.zeros((2, 6, 5, 5, 3), dtype=torch.uint8), 'spp_imgs', lead=(1, 2)) == ((2, 6), 5, 5)
    for shape, lead in (((2, 3, 5, 7), (1,)), ((5, 7, 3), (1,)), ((1, 2, 6, 5, 5, 3), (1, 2)), ((2, 6, 3, 5, 5), (1, 2))):
        with pytest.raises(ValueError):
            model._image_dims(torch.zeros(shape, dtype=torch.uint8), 'img', lead=lead)
    model.set_input_norm(lut=model.input_lut * 2)
    assert model.input_lut[0, 0] == np.float32(2) * ops.input_lut(par['mean'], par['std'])[0, 0]
    model.set_input_norm()
    assert model.input_lut is None
    # no table: nothing is judged (a uint8 NCHW tensor is cast as it always was)
    assert model._image_dims(torch.zeros((2, 3, 5, 7), dtype=torch.uint8), 'qry_img') == ((2,), 5, 7)
