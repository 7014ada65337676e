"""uint8 image input on the GPU: ``u8hwc3_to_nhwc4_kernel`` against ``nchw3_to_nhwc4`` of the host-normalised image bit
for bit, and the detector fed decoded pixels against the detector fed the data loader's float tensors, byte for byte
(eager, graph replay, cached support code, mixed dtypes, a changed table, training losses)."""
import numpy as np
import pytest
import torch

from fgn_amd import ops
from fgn_amd.episodes import collate
from fgn_amd.fewshot_ds import ClutteredCharsFewShotISEG

pytestmark = pytest.mark.gpu

N_WAYS, K_SHOTS, IMG, SPP = 3, 2, 128, 64
CH = np.arange(3)
# a clearly different table per channel (a channel mix-up cannot cancel)
LUT = ops.input_lut((0.11, 0.52, 0.93), (0.21, 0.34, 0.47))


def _ibits(t):
    return t.contiguous().view(torch.int32)


def _want(x_u8: np.ndarray, lut: np.ndarray) -> torch.Tensor:
    """The float path: host-normalised NCHW image -> nchw3_to_nhwc4."""
    nchw = np.ascontiguousarray(lut[CH, x_u8].transpose(0, 3, 1, 2))
    return ops.nchw3_to_nhwc4(torch.from_numpy(nchw).cuda())


def _check(x_dev: torch.Tensor, x_host: np.ndarray, lut=LUT):
    got = ops.u8hwc3_to_nhwc4(x_dev, torch.from_numpy(lut).cuda())
    want = _want(x_host, lut)
    assert got.shape == want.shape and got.dtype == torch.float32
    assert torch.equal(_ibits(got), _ibits(want))
    assert int(_ibits(got[..., 3]).abs().max()) == 0                                # +0.0, not -0.0
    return got


def _pixels(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, size=shape + (3,), dtype=np.uint8)


# one pass of the grid-stride loop covers ops.U8_PIXELS_PER_PASS pixels: the last shape needs a second pass of the 4-pixel
# loop and leaves a tail of 2
BIG_W = 2047
BIG_H = ops.U8_PIXELS_PER_PASS // BIG_W + 2


@pytest.mark.parametrize('shape', [(1, 1, 1), (1, 1, 3), (1, 3, 5), (2, 7, 9), (1, 16, 48), (1, BIG_H, BIG_W)])
def test_kernel_is_bitwise_the_float_path(shape):
    x = _pixels(shape, sum(shape))
    if shape == (1, 16, 48):          # all 256 values in every channel, in another order per channel
        v = np.arange(768) % 256
        x = np.stack([v, (v * 7 + 3) % 256, 255 - v], -1).astype(np.uint8).reshape(1, 16, 48, 3)
        assert all(len(np.unique(x[..., c])) == 256 for c in range(3))
    if shape[1] == BIG_H:
        assert x.size // 3 > ops.U8_PIXELS_PER_PASS and (x.size // 3) % 4
    _check(torch.from_numpy(x).cuda(), x)


@pytest.mark.parametrize('offset', [1, 2, 3])
@pytest.mark.parametrize('shape', [(2, 7, 9), (1, 513, 1025)])
def test_kernel_takes_views_that_are_not_dword_aligned(offset, shape):
    """A sliced uint8 view: every pixel goes the pixel-per-lane way; (1,513,1025) is more than one pass of THAT loop
    (a quarter of the pixels of the 4-pixel loop's pass)."""
    x = _pixels(shape, 40 + offset)
    if shape[1] == 513:
        assert x.size // 3 > ops.U8_PIXELS_PER_PASS // 4
    buf = torch.zeros(x.size + 8, dtype=torch.uint8, device='cuda')
    view = buf[offset:offset + x.size].view(x.shape)
    view.copy_(torch.from_numpy(x))
    assert view.is_contiguous() and view.data_ptr() % 4 == offset
    _check(view, x)
    assert int(buf[:offset].max()) == 0 and int(buf[offset + x.size:].max()) == 0


def test_kernel_empty_batch_and_null_pointers():
    x = torch.zeros((0, 4, 5, 3), dtype=torch.uint8, device='cuda')
    lut = torch.from_numpy(LUT).cuda()
    assert tuple(ops.u8hwc3_to_nhwc4(x, lut).shape) == (0, 4, 5, 4)
    from fgn_amd import lib
    L = lib.load()
    some = torch.zeros(16, dtype=torch.float32, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    assert L.fgn_u8hwc3_to_nhwc4_f32(some.data_ptr(), lut.data_ptr(), some.data_ptr(), 0, 4, 5, st) == 0
    for args in ((None, lut.data_ptr(), some.data_ptr()), (some.data_ptr(), None, some.data_ptr()),
                 (some.data_ptr(), lut.data_ptr(), None)):
        assert L.fgn_u8hwc3_to_nhwc4_f32(*args, 1, 1, 1, st) == -2
    torch.cuda.synchronize()
    assert float(some.abs().max()) == 0
    with pytest.raises(lib.FgnHipError):
        ops.u8hwc3_to_nhwc4(torch.zeros((1, 3, 4, 5), dtype=torch.uint8, device='cuda'), lut)       # NCHW
    with pytest.raises(lib.FgnHipError):
        ops.u8hwc3_to_nhwc4(torch.zeros((1, 4, 5, 3), dtype=torch.uint8, device='cuda'), lut[:, :255].contiguous())


# ------------------------------------------------------------------------------------------------ end to end
KEYS = ('dt_scores', 'dt_bboxes', 'dt_cat_ids')


def _model():
    from fgn_amd.config import tiny_config
    from fgn_amd.detector import FGN
    from fgn_amd.weights import init_state_dict
    cfg = tiny_config(N_WAYS, K_SHOTS, width_div=2)
    return FGN(N_WAYS, K_SHOTS, backbone=cfg['backbone'], rpn_head=cfg['rpn_head'], roi_head=cfg['roi_head'],
               test_cfg=cfg['test_cfg'], state_dict=init_state_dict(cfg, 0))


class _Env:
    """One model, one float / uint8 dataset pair, and the float path's results - computed once per batch, eagerly,
    before any table is set (the parent's behaviour) - shared by the tests below."""

    def __init__(self):
        kw = dict(dataset='MNISTISEG', n_ways=N_WAYS, k_shots=K_SHOTS, n_imgs=8, img_size=IMG, spp_img_size=SPP)
        self.ds_f, self.ds_u = ClutteredCharsFewShotISEG(**kw), ClutteredCharsFewShotISEG(**kw, raw_uint8=True)
        self.model = _model()
        self._ref = {}

    def reset(self):
        m = self.model
        m.use_graphs = False
        m.transfer_mode = 0
        m.use_merged_backbone = m.use_merged_support_head = True
        m.set_input_norm(**self.ds_u.input_norm)
        return m

    def pair(self, first, B):
        idx = range(first, first + B)
        return collate([self.ds_f[i] for i in idx]), collate([self.ds_u[i] for i in idx])

    def ref(self, first, B):
        if (first, B) not in self._ref:
            m = self.reset()
            m.set_input_norm()
            self._ref[first, B] = m.simple_test(**self.pair(first, B)[0], rescale=True)
            self.reset()
        return self._ref[first, B]


@pytest.fixture(scope='module')
def env():
    return _Env()


def _same(want, got, detections=True):
    assert len(want) == len(got)
    for a, b in zip(want, got):
        if detections:
            assert len(a['dt_scores']) > 0
        for k in KEYS:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
        assert a['dt_isegmaps_rle'] == b['dt_isegmaps_rle']
        assert a['qry_isegmaps_rle'] == b['qry_isegmaps_rle']


@pytest.mark.parametrize('B', [1, 2])
def test_simple_test_on_pixels_is_bytewise_the_float_path(env, B):
    want = env.ref(0, B)
    m = env.reset()
    bf, bu = env.pair(0, B)
    assert bu['qry_img'].dtype == torch.uint8 and tuple(bu['qry_img'].shape) == (B, IMG, IMG, 3)
    assert tuple(bu['spp_imgs'].shape) == (B, N_WAYS * K_SHOTS, SPP, SPP, 3)
    _same(want, m.simple_test(**bu, rescale=True))
    # float tensors still go the NCHW way with a table set; and a float query with pixel supports is legal
    _same(want, m.simple_test(**bf, rescale=True))
    _same(want, m.simple_test(**dict(bf, spp_imgs=bu['spp_imgs']), rescale=True))
    _same(want, m.simple_test(**dict(bu, spp_imgs=bf['spp_imgs']), rescale=True))
    # the separate-launch forms of the backbone and the shared head
    m.use_merged_backbone = m.use_merged_support_head = False
    sep_f = m.simple_test(**bf, rescale=True)
    _same(sep_f, m.simple_test(**bu, rescale=True))


@pytest.mark.parametrize('B', [1, 2])
def test_graph_replay_on_pixels(env, B):
    """Two different batches through ONE captured graph whose static image buffers are uint8."""
    want = [env.ref(0, B), env.ref(2, B)]
    m = env.reset()
    m.use_graphs = True
    for rep in range(2):
        for w, first in zip(want, (0, 2)):
            _same(w, m.simple_test(**env.pair(first, B)[1], rescale=True))
    assert len(m._graphs) == 1
    ge = next(iter(m._graphs.values()))
    assert ge.static['qry_img'].dtype == torch.uint8 and ge.static['spp_imgs'].dtype == torch.uint8
    assert tuple(ge.static['qry_img'].shape) == (B, IMG, IMG, 3)


def test_pinned_pixels_go_straight_into_the_static_buffers(env):
    """Transfers on the caller stream (``transfer_stream(3)``): host tensors are copied INTO the graph's static
    buffers - the uint8 ones as uint8."""
    want = [env.ref(0, 1), env.ref(2, 1)]
    m = env.reset()
    m.use_graphs = True
    m.transfer_mode = 3
    pin = lambda b: {k: (v.pin_memory() if isinstance(v, torch.Tensor) else v) for k, v in b.items()}
    b0, b2 = pin(env.pair(0, 1)[1]), pin(env.pair(2, 1)[1])
    _same(want[0], m.simple_test(**b0, rescale=True))
    _same(want[1], m.simple_test(**b2, rescale=True))
    _same(want[0], m.simple_test(**b0, rescale=True))
    assert len(m._graphs) == 1
    ge = next(iter(m._graphs.values()))
    torch.cuda.synchronize()
    for k in ('qry_img', 'spp_imgs'):
        assert ge.static[k].dtype == torch.uint8 and torch.equal(ge.static[k].cpu(), b0[k])
    ins = {k: b2[k] for k in ('qry_img', 'spp_imgs', 'spp_bboxes', 'spp_isegmaps')}
    main = torch.cuda.current_stream()
    out, _, ready = m._upload(ins, None, torch.device('cuda', torch.cuda.current_device()), main, into=ge.static)
    for k in ins:
        assert out[k] is ge.static[k], k
    torch.cuda.synchronize()
    assert torch.equal(ge.static['qry_img'].cpu(), b2['qry_img'])
    m.transfer_mode = 0


def test_support_code_from_pixel_supports(env):
    m = env.reset()
    for B in (1, 2):
        bf, bu = env.pair(4, B)
        q = lambda b: {k: v for k, v in b.items() if k not in ('spp_imgs', 'spp_bboxes', 'spp_isegmaps')}
        spp = lambda b: [b[k][0] if B == 1 else b[k] for k in ('spp_imgs', 'spp_bboxes', 'spp_isegmaps')]
        if B == 1:
            assert tuple(spp(bu)[0].shape) == (N_WAYS * K_SHOTS, SPP, SPP, 3)       # the 4-D form, as for floats
        code_f, code_u = m.encode_supports(*spp(bf)), m.encode_supports(*spp(bu))
        for k in ('vec', 'S', 'cat_mean_mp'):
            assert torch.equal(_ibits(code_f[k]), _ibits(code_u[k])), k
        want = m.simple_test(**q(bf), support_code=code_f, rescale=True)
        _same(want, m.simple_test(**q(bu), support_code=code_u, rescale=True))
        _same(want, m.simple_test(**q(bf), support_code=code_u, rescale=True))
        m.use_graphs = True
        _same(want, m.simple_test(**q(bu), support_code=code_u, rescale=True))
        _same(want, m.simple_test(**q(bu), support_code=code_u, rescale=True))
        m.use_graphs = False


def test_another_table_after_a_replay_is_followed(env):
    old = env.ref(0, 1)
    m = env.reset()
    m.use_graphs = True
    bu = env.pair(0, 1)[1]
    _same(old, m.simple_test(**bu, rescale=True))
    _same(old, m.simple_test(**bu, rescale=True))           # a replay
    assert len(m._graphs) == 1
    mean, std = np.float32([0.5, 0.45, 0.55]), np.float32([0.25, 0.3, 0.2])
    m.set_input_norm(mean=mean, std=std)
    assert m._graphs == {}
    got = m.simple_test(**bu, rescale=True)
    got_again = m.simple_test(**bu, rescale=True)
    # the float path normalised the new way
    env.ds_f.mean, env.ds_f.std = mean, std
    try:
        bf = collate([env.ds_f[0]])
    finally:
        env.ds_f.mean, env.ds_f.std = env.ds_u.mean.copy(), env.ds_u.std.copy()
    m.use_graphs = False
    m.set_input_norm()
    want = m.simple_test(**bf, rescale=True)
    _same(want, got, detections=False)
    _same(want, got_again, detections=False)
    assert got[0]['dt_scores'].tobytes() != old[0]['dt_scores'].tobytes()


def test_wrong_pixel_layouts_are_refused(env):
    m = env.reset()
    bf, bu = env.pair(0, 1)
    nchw = bu['qry_img'].permute(0, 3, 1, 2).contiguous()
    with pytest.raises(ValueError):
        m.simple_test(**dict(bu, qry_img=nchw), rescale=True)
    with pytest.raises(ValueError):
        m.simple_test(**dict(bu, spp_imgs=bu['spp_imgs'].permute(0, 1, 4, 2, 3).contiguous()), rescale=True)
    with pytest.raises(ValueError):
        m.encode_supports(bu['spp_imgs'][0].permute(0, 3, 1, 2).contiguous(), bu['spp_bboxes'][0], bu['spp_isegmaps'][0])
    m.use_graphs = True
    with pytest.raises(ValueError):
        m.simple_test(**dict(bu, qry_img=nchw), rescale=True)
    assert m._graphs == {}
    m.use_graphs = False
    with pytest.raises(ValueError):
        m.forward_train(**dict(bu, qry_img=nchw))
    # no table: a uint8 NCHW tensor is cast as it always was (raw 0..255 floats)
    m.set_input_norm()
    assert torch.equal(_ibits(m._stem_input(nchw)), _ibits(ops.nchw3_to_nhwc4(nchw.float().cuda())))


def test_forward_train_on_pixels_gives_the_same_losses():
    env = _Env()
    m = env.reset()
    bf, bu = env.pair(0, 2)
    losses = []
    for b in (bf, bu, dict(bf, spp_imgs=bu['spp_imgs'])):
        m._PT = None                                    # fresh running statistics
        g = torch.Generator().manual_seed(3)
        torch.manual_seed(3)
        losses.append(m.forward_train(**b, perm_fn=lambda n: torch.randperm(n, generator=g)))
    val = lambda v: torch.as_tensor(v[0] if isinstance(v, list) else v).detach().cpu().reshape(-1)
    for other in losses[1:]:
        assert set(other) == set(losses[0])
        for k in losses[0]:
            a, b = val(losses[0][k]), val(other[k])
            assert a.dtype == b.dtype and a.numpy().tobytes() == b.numpy().tobytes(), k
    assert all(np.isfinite(float(val(v)[0])) for v in losses[0].values())
    assert float(val(losses[0]['loss_rpn_cls'])[0]) > 0 and float(val(losses[0]['loss_cls'])[0]) > 0
