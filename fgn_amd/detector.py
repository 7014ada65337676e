"""FGN detector: the drop-in boundary of the hot path.

Mirrors the reference's detector API (subprojects/sp02_omniiseg_fgn_mmdet/fgn.py:28-303):
``FGN(n_ways, k_shots, backbone=..., rpn_head=..., roi_head=..., train_cfg=..., test_cfg=...)``,
``forward(return_loss, **batch)``, ``simple_test(**batch, rescale=True)`` with the
FewShotISEG batch dict in and the per-image result dicts out (same keys, numpy values,
YXYX boxes, COCO RLE masks).  The constructor accepts the reference's mmcv-style config
dicts (fgn_r50_c4_densecl.py:13-186) unchanged.

Host code is Python/PyTorch plumbing (device memory, streams).  Every arithmetic step
runs in libfgn_hip.so (hand-written gfx950 HIP kernels, include/fgn_hip.h); there is no
eager/CPU fallback: without the library or without a GPU ``simple_test`` raises.

Data layout in HBM: all feature maps NHWC fp32; RoI tensors [R,7,7,C] (a RoI is an
"image" of the conv kernel); weights pre-packed [CoutPad][KH][KW][Cin]; eval-mode BN
folded into a per-channel scale/shift epilogue.  Data-dependent counts (proposals,
detections) stay in device int32 counters consumed by the kernels, so an episode runs
without host synchronisation until the final device-to-host copy of the results.
"""
from __future__ import annotations

import copy
import os
from collections import OrderedDict
from typing import Dict, List, NamedTuple, Optional, Union

import numpy as np
import torch

from . import config as _config
from . import maskforms, ops, rle
from .weights import backbone_state_from_pretrained, init_state_dict


# ------------------------------------------------------------------------------------------
# reference-style (mmcv) config -> flat config
# ------------------------------------------------------------------------------------------
_R50_BLOCKS = (3, 4, 6, 3)


def normalise_config(n_ways, k_shots, backbone=None, rpn_head=None, roi_head=None, test_cfg=None,
                     train_cfg=None) -> dict:
    """Accept either this package's flat dicts or the reference's mmcv config dicts."""
    cfg = _config.fgn_r50_c4_config(n_ways, k_shots)
    if backbone:
        if 'stage_blocks' in backbone:
            cfg['backbone'].update(backbone)
        else:   # mmdet ResNet dict (fgn_r50_c4_densecl.py:15-42); layer4 is dropped (main.py:403-405)
            depth = backbone.get('depth', 50)
            if depth not in (18, 50):
                raise NotImplementedError('ResNet-50-C4 (both reference configs) and the ResNet-18 extension are built')
            last = max(backbone.get('out_indices', (2,)))
            norm = backbone.get('norm_cfg', dict(type='BN'))
            if norm.get('type', 'BN') not in ('BN', 'GN'):
                raise NotImplementedError(f"norm_cfg {norm.get('type')!r}")
            if depth == 18 and (norm.get('type', 'BN') != 'BN' or backbone.get('deep_stem') or backbone.get('avg_down')):
                raise NotImplementedError('ResNet-18 extension: frozen-BN BasicBlock stages only')
            cfg['backbone'].update(depth=depth, block='basic' if depth == 18 else 'bottleneck')
            cfg['backbone'].update(stage_blocks=((2, 2, 2, 2) if depth == 18 else _R50_BLOCKS)[:last + 1],
                                   stage_planes=(64, 128, 256, 512)[:last + 1],
                                   strides=tuple(backbone.get('strides', (1, 2, 2, 2)))[:last + 1],
                                   # fgn_r50_c4_scratch.py:16-23
                                   deep_stem=bool(backbone.get('deep_stem', False)),
                                   avg_down=bool(backbone.get('avg_down', False)),
                                   norm=norm.get('type', 'BN'), gn_groups=norm.get('num_groups', 32),
                                   ref_num_stages=int(backbone.get('num_stages', 4)))
    if rpn_head:
        r = cfg['rpn_head']
        if 'anchor_generator' in rpn_head:
            ag, bc = rpn_head['anchor_generator'], rpn_head.get('bbox_coder', {})
            r.update(in_channels=rpn_head.get('in_channels', r['in_channels']),
                     feat_channels=rpn_head.get('feat_channels', r['feat_channels']),
                     anchor_scales=tuple(ag['scales']), anchor_ratios=tuple(ag['ratios']),
                     anchor_stride=ag['strides'][0],
                     target_means=tuple(bc.get('target_means', r['target_means'])),
                     target_stds=tuple(bc.get('target_stds', r['target_stds'])))
        else:
            r.update(rpn_head)
    if roi_head:
        h = cfg['roi_head']
        if 'bbox_roi_extractor' in roi_head:
            ex = roi_head['bbox_roi_extractor']
            h.update(roi_out_size=ex['roi_layer']['output_size'],
                     roi_sampling_ratio=ex['roi_layer'].get('sampling_ratio', 0),
                     featmap_stride=ex['featmap_strides'][0])
            bh, mh = roi_head.get('bbox_head', {}), roi_head.get('mask_head', {})
            bc = bh.get('bbox_coder', {})
            h['bbox_head'].update(in_channels=bh.get('in_channels', 1024), num_classes=bh.get('num_classes', 1),
                                  target_means=tuple(bc.get('target_means', (0., 0., 0., 0.))),
                                  target_stds=tuple(bc.get('target_stds', (.1, .1, .2, .2))))
            h['mask_head'].update({k: mh[k] for k in ('num_convs', 'in_channels', 'conv_out_channels',
                                                      'num_classes') if k in mh})
        else:
            for k, v in roi_head.items():
                if isinstance(v, dict) and k in h:
                    h[k].update(v)
                else:
                    h[k] = v
    if test_cfg:
        t = cfg['test_cfg']
        for part in ('rpn', 'rcnn'):
            src = dict(test_cfg.get(part, {}))
            if 'nms' in src:
                src['nms_iou_threshold'] = src.pop('nms')['iou_threshold']
            t[part].update(src)
    if train_cfg:
        # mmdet layout (fgn_r50_c4_densecl.py:131-171): assigner / sampler sub-dicts are flattened
        t = cfg['train_cfg']
        for part in ('rpn', 'rcnn', 'rpn_proposal'):
            src = dict(train_cfg.get(part, {}))
            for sub, typ in (('assigner', 'MaxIoUAssigner'), ('sampler', 'RandomSampler')):
                d = dict(src.pop(sub, {}))
                if d.pop('type', typ) != typ:
                    raise NotImplementedError(f'train_cfg.{part}.{sub}: only {typ} (both reference configs)')
                d.pop('ignore_iof_thr', None)
                src.update(d)
            if 'nms' in src:
                src['nms_iou_threshold'] = src.pop('nms')['iou_threshold']
            src.pop('debug', None)
            t[part].update(src)
    return cfg


# ------------------------------------------------------------------------------------------
class _Bottleneck:
    def __init__(self, sd, prefix, stride, eps, winograd=0):
        bn = lambda n: {k: sd[f'{prefix}.{n}.{k}'] for k in ('weight', 'bias', 'running_mean', 'running_var')}
        self.conv1 = ops.pack_conv(sd[prefix + '.conv1.weight'], bn=bn('bn1'), relu=True, eps=eps)
        self.conv2 = ops.pack_conv(sd[prefix + '.conv2.weight'], bn=bn('bn2'), stride=stride, pad=1, relu=True,
                                   eps=eps)
        # Winograd form of a stride-1 3x3 (F(4x4,3x3): 4x fewer MFMA passes); chosen per call by ops.winograd_pays
        w2 = sd[prefix + '.conv2.weight']
        self.conv2_wg = ops.pack_winograd(w2, bn=bn('bn2'), relu=True, eps=eps, m=winograd) \
            if winograd and stride == 1 and w2.shape[1] % 32 == 0 and w2.shape[0] % 4 == 0 else None
        self.conv3 = ops.pack_conv(sd[prefix + '.conv3.weight'], bn=bn('bn3'), relu=True, eps=eps)
        self.down = None
        self.conv3_dual = None
        if (prefix + '.downsample.0.weight') in sd:
            dbn = {k: sd[f'{prefix}.downsample.1.{k}'] for k in ('weight', 'bias', 'running_mean', 'running_var')}
            wd = sd[prefix + '.downsample.0.weight']
            self.down = ops.pack_conv(wd, bn=dbn, stride=stride, eps=eps)
            # first block of a stage: conv3 + bn3 and the 1x1 shortcut conv + bn as ONE dual-operand K loop - no launch
            # and no [rows, Cout] round trip for the shortcut (ops.conv1x1_dual).  Stride 1 (layer1.0): both read the
            # same pixels; stride 2 (layer2.0, layer3.0): the shortcut's rows come through a row table (_strided_rows)
            w3 = sd[prefix + '.conv3.weight']
            if ops.FUSED_SHORTCUT and stride in ops.FUSED_SHORTCUT_STRIDES and tuple(wd.shape[2:]) == (1, 1) and \
                    w3.shape[1] % 32 == 0 and wd.shape[1] % 32 == 0 and w3.shape[0] % 4 == 0:
                self.conv3_dual = ops.pack_conv_dual(w3, bn('bn3'), wd, dbn, relu=True, eps=eps)

    def layers(self):
        return [l for l in (self.conv1, self.conv2, self.conv3, self.down, self.conv2_wg, self.conv3_dual) if l is not None]

    def __call__(self, x, n_img_dev=None, y1=None):
        """``y1``: the output of conv1 (+BN+ReLU) when the caller already has it (shared_head entry)."""
        fused = self.conv3_dual is not None and n_img_dev is None
        idt = x if (self.down is None or fused) else ops.conv2d(x, self.down, n_img_dev=n_img_dev)
        y = y1 if y1 is not None else ops.conv2d(x, self.conv1, n_img_dev=n_img_dev)
        if self.conv2_wg is not None and \
                ops.winograd_pays(y.shape[0], y.shape[1], y.shape[2], self.conv2_wg.cin, self.conv2_wg.cout,
                                  self.conv2_wg.m):
            y = ops.conv3x3_winograd(y, self.conv2_wg, n_img_dev=n_img_dev)
        else:
            y = ops.conv2d(y, self.conv2, n_img_dev=n_img_dev)
        if fused:                                                              # relu(bn3(conv3(y)) + bn_d(conv_d(x)))
            rows = None if self.down.stride == 1 else _strided_rows([tuple(x.shape[:3])], self.down.stride, x.device)
            return ops.conv1x1_dual(y, x, self.conv3_dual, x2_rows=rows)
        return ops.conv2d(y, self.conv3, residual=idt, n_img_dev=n_img_dev)   # relu(bn3(conv3) + identity)


_ROW_TABLES: dict = {}


def _strided_rows(shapes, stride, device):
    """``ops.strided_rows`` cached per (geometry, stride, device): built once on the host, outside any graph capture of
    the same geometry (the eager run that precedes a capture fills the cache)."""
    key = (tuple(shapes), int(stride), str(device))
    t = _ROW_TABLES.get(key)
    if t is None:
        t = _ROW_TABLES[key] = ops.strided_rows(shapes, stride, device)
    return t


class _Pair:
    """Two NHWC tensors (query map, support maps) that live in ONE [M_q + M_s, C] buffer, so that the layers whose
    work does not depend on the spatial structure (1x1 / stride 1 convolutions, the grouped Winograd GEMM) run as one
    launch over all rows."""

    def __init__(self, q_shape, s_shape, c, device):
        self.mq = q_shape[0] * q_shape[1] * q_shape[2]
        self.ms = s_shape[0] * s_shape[1] * s_shape[2]
        self.buf = torch.empty((self.mq + self.ms, c), device=device, dtype=torch.float32)
        self.q = self.buf[:self.mq].view(*q_shape, c)
        self.s = self.buf[self.mq:].view(*s_shape, c)

    @property
    def flat(self):
        return self.buf.view(1, self.mq + self.ms, 1, self.buf.shape[1])

    def like(self, c, q_hw=None, s_hw=None):
        qs = self.q.shape[:3] if q_hw is None else (self.q.shape[0],) + tuple(q_hw)
        ss = self.s.shape[:3] if s_hw is None else (self.s.shape[0],) + tuple(s_hw)
        return _Pair(tuple(qs), tuple(ss), c, self.buf.device)


USE_CONV_PAIR = os.environ.get('FGN_CONV_PAIR', '1') != '0'      # A/B knob: 0 = one launch per tensor


def _conv_pair(xq, xs, layer, out_q, out_s):
    """A convolution that strides over the spatial structure on the query map and the support maps: one two-tensor
    launch (ops.conv2d_pair), or one launch each."""
    if USE_CONV_PAIR and layer.cout % 4 == 0 and (layer.cin == 4 or layer.cin % 32 == 0):
        ops.conv2d_pair(xq, xs, layer, out_q, out_s)
    else:
        ops.conv2d(xq, layer, out=out_q)
        ops.conv2d(xs, layer, out=out_s)


def _bottleneck_pair(blk: '_Bottleneck', x: _Pair) -> _Pair:
    """``_Bottleneck.__call__`` on a query / support pair: merged launches for conv1, conv3 (+ residual), the
    stride-1 downsample and the Winograd GEMM; two-tensor launches for the strided convolutions and the transforms."""
    stride = blk.conv2.stride
    out_hw = lambda t: ((t.shape[1] - 1) // stride + 1, (t.shape[2] - 1) // stride + 1)
    fused = blk.conv3_dual is not None
    if blk.down is None or fused:
        idt = x
    else:
        idt = x.like(blk.down.cout, out_hw(x.q), out_hw(x.s))
        if blk.down.stride == 1:
            ops.conv2d(x.flat, blk.down, out=idt.flat)
        else:
            _conv_pair(x.q, x.s, blk.down, idt.q, idt.s)
    y1 = x.like(blk.conv1.cout)
    ops.conv2d(x.flat, blk.conv1, out=y1.flat)
    y2 = x.like(blk.conv2.cout, out_hw(x.q), out_hw(x.s))
    wg = blk.conv2_wg
    if wg is not None and ops.winograd_pays(1, (y1.mq + y1.ms) // 64 + 1, 64, wg.cin, wg.cout, wg.m):
        ops.conv3x3_winograd_multi([y1.q, y1.s], wg, [y2.q, y2.s])
    else:
        _conv_pair(y1.q, y1.s, blk.conv2, y2.q, y2.s)
    out = y2.like(blk.conv3.cout)
    if fused:       # (stride 1: y2 and x hold the same rows; stride 2: the shortcut's rows through a row table)
        rows = None if stride == 1 else _strided_rows([tuple(x.q.shape[:3]), tuple(x.s.shape[:3])], stride, x.buf.device)
        ops.conv1x1_dual(y2.flat, x.flat, blk.conv3_dual, out=out.flat, x2_rows=rows)
    else:
        ops.conv2d(y2.flat, blk.conv3, residual=idt.flat, out=out.flat)
    return out


class _BasicBlock:
    """mmdet BasicBlock of the ResNet-18 extension (config.fgn_r18_c4_config): conv3x3(stride)+BN+ReLU, conv3x3+BN,
    + identity, ReLU.  conv1 takes the Winograd form when it has stride 1 and pays; conv2 carries the residual in
    the epilogue of the direct kernel."""

    def __init__(self, sd, prefix, stride, eps, winograd=0):
        bn = lambda n: {k: sd[f'{prefix}.{n}.{k}'] for k in ('weight', 'bias', 'running_mean', 'running_var')}
        w1 = sd[prefix + '.conv1.weight']
        self.conv1 = ops.pack_conv(w1, bn=bn('bn1'), stride=stride, pad=1, relu=True, eps=eps)
        self.conv1_wg = ops.pack_winograd(w1, bn=bn('bn1'), relu=True, eps=eps, m=winograd) \
            if winograd and stride == 1 and w1.shape[1] % 32 == 0 and w1.shape[0] % 4 == 0 else None
        self.conv2 = ops.pack_conv(sd[prefix + '.conv2.weight'], bn=bn('bn2'), pad=1, relu=True, eps=eps)
        self.down = None
        if (prefix + '.downsample.0.weight') in sd:
            dbn = {k: sd[f'{prefix}.downsample.1.{k}'] for k in ('weight', 'bias', 'running_mean', 'running_var')}
            self.down = ops.pack_conv(sd[prefix + '.downsample.0.weight'], bn=dbn, stride=stride, eps=eps)

    def layers(self):
        return [l for l in (self.conv1, self.conv1_wg, self.conv2, self.down) if l is not None]

    def __call__(self, x, n_img_dev=None):
        idt = x if self.down is None else ops.conv2d(x, self.down, n_img_dev=n_img_dev)
        wg = self.conv1_wg
        if wg is not None and ops.winograd_pays(x.shape[0], x.shape[1], x.shape[2], wg.cin, wg.cout, wg.m):
            y = ops.conv3x3_winograd(x, wg, n_img_dev=n_img_dev)
        else:
            y = ops.conv2d(x, self.conv1, n_img_dev=n_img_dev)
        return ops.conv2d(y, self.conv2, residual=idt, n_img_dev=n_img_dev)   # relu(bn2(conv2) + identity)


class _BottleneckGN:
    """Bottleneck of the from-scratch backbone (fgn_r50_c4_scratch.py:16-25): conv -> GroupNorm -> ReLU;
    the norm cannot fold into the conv epilogue, so every conv is followed by the GN passes.  Shortcut
    under avg_down: [2x2 average pool if strided] -> 1x1 conv (stride 1) -> GN."""

    def __init__(self, sd, prefix, stride, groups, eps, avg_down):
        self.groups, self.eps = groups, eps
        self.conv1 = ops.pack_conv(sd[prefix + '.conv1.weight'])
        self.conv2 = ops.pack_conv(sd[prefix + '.conv2.weight'], stride=stride, pad=1)
        self.conv3 = ops.pack_conv(sd[prefix + '.conv3.weight'])
        self.gn = [[sd[f'{prefix}.gn{i}.weight'].clone(), sd[f'{prefix}.gn{i}.bias'].clone()] for i in (1, 2, 3)]
        self.pooled = bool(avg_down) and stride != 1
        if self.pooled and stride != 2:
            raise NotImplementedError('avg_down shortcut: only stride 2')
        i = 1 if self.pooled else 0
        # (mmdet's ResLayer may put the AvgPool2d in front of a stride-1 shortcut too - kernel 1, the identity - which
        # shifts the conv / norm to downsample.1 / .2 in layer1 as well: unverifiable here (mmdet 2.18 is absent), so a
        # checkpoint in either key layout loads)
        if f'{prefix}.downsample.{i}.weight' not in sd and f'{prefix}.downsample.{1 - i}.weight' in sd:
            i = 1 - i
        self.down = None
        if f'{prefix}.downsample.{i}.weight' in sd:
            self.down = ops.pack_conv(sd[f'{prefix}.downsample.{i}.weight'], stride=1 if avg_down else stride)
            self.gn.append([sd[f'{prefix}.downsample.{i + 1}.weight'].clone(),
                            sd[f'{prefix}.downsample.{i + 1}.bias'].clone()])

    def layers(self):
        return [l for l in (self.conv1, self.conv2, self.conv3, self.down) if l is not None]

    def to(self, device):
        for l in self.layers():
            l.to(device)
        self.gn = [[t.float().contiguous().to(device) for t in pair] for pair in self.gn]
        return self

    def _norm(self, x, i, relu, residual=None):
        return ops.group_norm(x, self.gn[i][0], self.gn[i][1], self.groups, self.eps, relu=relu, residual=residual,
                              inplace=True)

    def __call__(self, x, n_img_dev=None):
        idt = x
        if self.down is not None:
            idt = self._norm(ops.conv2d(ops.avgpool2x2(x) if self.pooled else x, self.down), 3, False)
        y = self._norm(ops.conv2d(x, self.conv1), 0, True)
        y = self._norm(ops.conv2d(y, self.conv2), 1, True)
        return self._norm(ops.conv2d(y, self.conv3), 2, True, residual=idt)   # relu(gn3(conv3) + identity)


class _ResultRecord:
    """Every per-image output of one batch in ONE buffer (device, or its pinned host mirror): the selection / mask
    kernels write straight into its views and ONE device-to-host copy moves it (round 5: the nine small copies per
    episode it replaces were ~6 us blit kernels each on the caller stream).  Layout, 256-byte aligned fields:
    [n_dets | rle_len | rle_overflow | mask_prob] (the zero-initialised head) | det_bboxes | det_labels | rle bytes."""

    def __init__(self, batch: int, max_det: int, mask_size: int, device=None, pinned: bool = False):
        self.key = (batch, max_det, mask_size, ops.RLE_BYTE_CAP)
        off, spec = 0, []
        for name, shape, dtype in (('cnt', (batch, 1), torch.int32), ('rle_len', (batch, max_det), torch.int32),
                                   ('rle_ovf', (batch, max_det), torch.int32),
                                   ('prob', (batch, max_det, mask_size, mask_size), torch.float32), (None, None, None),
                                   ('det', (batch, max_det, 5), torch.float32), ('lab', (batch, max_det), torch.int64),
                                   ('rle', (batch, max_det, ops.RLE_BYTE_CAP), torch.uint8)):
            if name is None:
                self.zero_bytes = off
                continue
            n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
            spec.append((name, shape, dtype, off, n))
            off = (off + n + 255) // 256 * 256
        self.nbytes = off
        self.buf = torch.empty(off, dtype=torch.uint8, pin_memory=True) if pinned else \
            torch.empty(off, dtype=torch.uint8, device=device)
        for name, shape, dtype, o, n in spec:
            setattr(self, name, self.buf[o:o + n].view(dtype).view(*shape))

    def clear_head(self) -> None:
        self.buf[:self.zero_bytes].zero_()


class _GraphedEpisode:
    """The launch sequence of ``FGN._detect_eager`` for one input geometry, captured once as a
    hipGraph (both HIP streams of the path fork from and join the capture stream).  Inputs are copied
    into static device buffers (this copy is the H2D step of fgn.py:79-108 when the batch arrives on
    the host), outputs live in static buffers that the next replay overwrites - so the replay waits
    for the previous download; that download (one copy of the batch's result record) carries every tensor
    ``pack_results`` may read."""
    CODE_KEYS = ('vec', 'S', 'cat_mean_mp')

    def __init__(self, model, ins: dict, img_shape, support_code, dev, phase_counter, form: '_InputForm'):
        self.static = {k: torch.empty(v.shape, dtype=v.dtype, device=dev) for k, v in ins.items()}
        self.slots = form.slots()   # rows of a configured capacity, whatever this batch needs: a batch fills their fronts
        for k, shape in self.slots.items():
            self.static[k] = torch.empty(shape, dtype=torch.uint8, device=dev)
        self.img_shape = torch.as_tensor(img_shape).cpu().clone()
        self.code = None
        if support_code is not None:
            self.code = dict(support_code)
            for k in self.CODE_KEYS:
                self.code[k] = support_code[k].clone()
        self.last_download = None
        for k, v in ins.items():
            self._copy_in(k, v)
        args = lambda: (form.query(self.static), form.supports(self.static), self.static.get('spp_bboxes'),
                        self.static.get('spp_isegmaps'), self.img_shape, self.code)
        # eager pass first: packs the weights, sets kernel attributes, sizes the allocator pools
        # (the eager run that precedes the capture sends no phase mark: every ``detect_device`` call bumps the caller's
        # counter exactly once - here through the replay that follows the capture)
        model._detect_eager(*args(), phase_counter=None, results_at_source=form.at_source)
        torch.cuda.current_stream().synchronize()
        self.graph = torch.cuda.CUDAGraph()
        # launch records of the dominant kernel (``FGN.stamp_capacity``; bench.py's roofline over the whole timed window):
        # the record of every conv_pw_persist_kernel launch is baked into the captured launch, each replay adds its span
        self.stamps, self.stamp_count = None, 0
        if model.stamp_capacity:
            self.stamps = ops.new_stamp_records(int(model.stamp_capacity), dev)
            torch.cuda.current_stream().synchronize()
            ops.arm_stamps(self.stamps)
        # thread-local capture mode: only this thread's calls are checked against the capture, so nothing another
        # thread does (the watchdog of an RCCL process group polling the all-gather of the previous step) can
        # invalidate it.  (The global mode passed the same test on this torch build; FGN_GRAPH_CAPTURE_MODE selects.)
        try:
            with torch.cuda.graph(self.graph, capture_error_mode=os.environ.get('FGN_GRAPH_CAPTURE_MODE', 'thread_local')):
                self.outs = model._detect_eager(*args(), phase_counter=phase_counter,
                                                results_at_source=form.at_source)
        finally:
            if self.stamps is not None:
                self.stamp_count = ops.arm_stamps(None)

    def _copy_in(self, k: str, v: torch.Tensor) -> None:
        if k in self.slots:         # [B, what the batch needs] into the front of the slot rows; the rest is never read
            self.static[k][:, :v.shape[1]].copy_(v, non_blocking=True)
        else:
            self.static[k].copy_(v, non_blocking=True)

    def run(self, model, ins: dict, support_code, main) -> list:
        for k, v in ins.items():
            if v is not self.static[k]:                # (already uploaded straight into the static buffer: detect_device)
                self._copy_in(k, v)
        if support_code is not None:
            for k in self.CODE_KEYS:
                if support_code[k].data_ptr() != self.code[k].data_ptr():
                    self.code[k].copy_(support_code[k], non_blocking=True)
        if self.last_download is not None:
            main.wait_event(self.last_download)       # static outputs are still being read by the copy stream
        self.graph.replay()
        # (the static outputs are views of the batch's result record: its one download carries everything pack_results
        # reads, the mask probabilities and boxes of the rare RLE-overflow fallback included)
        return [dict(d) for d in self.outs]          # detect_device queues the download and sets ``last_download``


def _host(v) -> np.ndarray:
    """A tensor, array or nested list as a host array."""
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def _gt_entries(qry_isegmaps, sizes, imgs=None):
    """``qry_isegmaps`` normalised once at the front (host only, nothing is queued): an entry in a compact form
    (``maskforms``: COCO RLE - the empty list included -, box + colour, COCO polygons) becomes its checked carrier at
    ``sizes[i]`` = (h, w) - a size that disagrees is a ValueError -, a dense entry stays as it is.  A colour carrier is
    bound to ``imgs[i]`` - the image's bytes [h,w,3] as they were handed over, which is what its mask is made from;
    ``imgs`` is None where the images are not bytes (float input), and a colour entry is refused then.  A bare nested
    list is never polygons - it reads as a dense mask, and one that is no [n,h,w] array of numbers is refused here.
    Without a compact entry the argument itself comes back."""
    if qry_isegmaps is None or not isinstance(qry_isegmaps, (list, tuple)):
        return qry_isegmaps
    forms = [maskforms.form_of(g) for g in qry_isegmaps]
    for i, g in enumerate(qry_isegmaps):
        if isinstance(g, (list, tuple)) and forms[i] is None:
            _dense_lists(g, f'qry_isegmaps[{i}]', sizes[i] if sizes is not None and i < len(sizes) else None)
    if all(f is None for f in forms):
        return qry_isegmaps
    if sizes is not None and len(sizes) != len(qry_isegmaps):
        raise ValueError(f'qry_isegmaps has {len(qry_isegmaps)} entries for {len(sizes)} images')
    out = []
    for i, (g, form) in enumerate(zip(qry_isegmaps, forms)):
        if form is maskforms.COLOR and imgs is None:
            raise ValueError(f'qry_isegmaps[{i}]: a box + colour entry is made into a mask from the image\'s bytes on '
                             f'the device: give qry_img as uint8 pixels (set_input_norm, with or without '
                             f'qry_resize_to), not as a normalised float tensor')
        out.append(g if form is None else form.check(g, None if sizes is None else sizes[i], f'qry_isegmaps[{i}]',
                                                     imgs[i] if form is maskforms.COLOR else None))
    return out


def _dense_lists(g, what: str, hw=None) -> None:
    """A mask entry given as nested lists that is no RLE reads as a dense mask: it must be an [n,h,w] array of numbers,
    at ``hw`` where that is known.  COCO's ``segmentation`` lists have the same nesting, which is why polygons never come
    bare."""
    try:
        a = np.asarray(g)
    except (ValueError, TypeError):
        a = None
    if a is None or a.ndim != 3 or a.dtype.kind not in 'biuf' or \
            (hw is not None and a.shape[0] and tuple(a.shape[1:]) != tuple(int(v) for v in hw)):
        raise ValueError(f"{what}: a nested list reads as a dense mask and must be an [n,h,w] array of numbers at its image's "
                         f"size{'' if hw is None else ' ' + str([int(v) for v in hw])}; polygons "
                         f"come as {{'polygons': [instance, ...]}} or a PolyMasks (fgn_amd.polygon), never as bare lists")


def _has_color(entries) -> bool:
    return isinstance(entries, (list, tuple)) and any(maskforms.form_of(g) is maskforms.COLOR for g in entries)


def _dense_supports_only(spp_isegmaps) -> None:
    """The plain support path takes the dense [B,N*K,S,S] tensor only: the supports are already cut, resized and
    padded there, and no dataset holds such masks as runs - nor is there a source image to derive a box + colour mask
    from."""
    flat = spp_isegmaps if isinstance(spp_isegmaps, (list, tuple)) else [spp_isegmaps]
    found = {maskforms.form_of_one(v) for m in flat for v in ([m, *m] if isinstance(m, (list, tuple)) else [m])}
    if maskforms.POLY in found:
        raise ValueError('spp_isegmaps: without spp_crop_to the supports are the dense [B,N*K,S,S] tensor; polygon masks '
                         'are taken in their source images\' frame, with spp_crop_to')
    if maskforms.COLOR in found:
        raise ValueError('spp_isegmaps: without spp_crop_to the supports are the dense [B,N*K,S,S] tensor; box + colour '
                         'masks are made from the instances\' source images, with spp_crop_to')
    if isinstance(spp_isegmaps, (list, tuple, dict, maskforms.RLE.carrier)):
        raise ValueError('spp_isegmaps: without spp_crop_to the supports are the dense [B,N*K,S,S] tensor; RLE masks '
                         'are taken at source size, with spp_crop_to')


def _number_rows(v, shapes: tuple, must: str) -> np.ndarray:
    """The rows of an augmentation argument as a host array: numbers, in one of ``shapes``."""
    a = _host(v)
    if a.dtype.kind not in 'iuf' or a.shape not in shapes:
        raise ValueError(f'{must}, got {a.dtype} {list(a.shape)}')
    return a


def _moved(t: tuple, dev):
    """A carrier with every tensor it holds on ``dev`` (None and the plain numbers stay)."""
    return t._make(v.to(dev, non_blocking=True) if isinstance(v, torch.Tensor) else v for v in t)


class _QueryPixels(NamedTuple):
    """Query images at their source size on the way to the stem (``qry_resize_to``): ``src`` uint8 [B, capacity], image b
    = [h_b, w_b, 3] pixels at the start of row b; ``hw`` int32 [B,2] = (h_b, w_b); (H, W) the network size; ``rec``
    (``qry_augment``) int32 [B,16], the records of ``fewshot_ds.query_augment_record`` (source size included), or None
    for the plain resize.  Stands where the ``qry_img`` tensor stands between ``detect_device`` / ``forward_train`` and
    ``_stem_input``; on that way only ``shape[0]``, ``to(device)``, ``dims`` (``FGN._image_dims``) and ``stem_input``
    (``FGN._stem_input``) are asked of a query, and those it answers."""
    src: torch.Tensor
    hw: torch.Tensor
    H: int
    W: int
    rec: Optional[torch.Tensor] = None

    @property
    def shape(self) -> tuple:
        return (self.src.shape[0], self.H, self.W, 3)

    @property
    def dims(self) -> tuple:
        return (int(self.src.shape[0]),), self.H, self.W

    def to(self, dev, *a, **kw) -> '_QueryPixels':
        return _moved(self, dev)

    def stem_input(self, lut: torch.Tensor) -> torch.Tensor:
        """The NHWC4 fp32 input of the stem, in one launch: resized, or warped by ``rec``, and normalised."""
        if self.rec is None:
            return ops.resize_u8_to_nhwc4(self.src.contiguous(), self.hw.contiguous(), lut, self.H, self.W)
        return ops.augment_u8_to_nhwc4(self.src.contiguous(), self.rec.contiguous(), lut, self.H, self.W)


class _SupportWindows(NamedTuple):
    """Support instances as windows of their source images on the way to ``_support_front`` (``spp_crop_to``): ``src``
    uint8 [n, capacity], instance i's image window [wh_i, ww_i, 3] at the start of row i; ``msk`` uint8 [n, mask capacity],
    its mask window; ``rec`` int32 [n,16], the records of ``fewshot_ds.support_geometry``; ``S`` the support size.  Stands
    where the ``spp_imgs`` tensor stands; ``spp_isegmaps`` is None beside it (the kernel makes the masks).  With an
    augmentation (``spp_augment`` / ``spp_photometric``): ``aug`` int32 [n,16], the records of
    ``fewshot_ds.query_augment_record`` at S -> S, and ``photo`` int32 [n,64], the records of
    ``fewshot_ds.query_photometric_record`` - or None where every instance's is neutral (no photometric launch); with
    ``spp_photometric_chain`` and an instance of two active operators, int32 [n,P,64], the records of
    ``fewshot_ds.photometric_chain_records``, for the chain kernel."""
    src: torch.Tensor
    msk: torch.Tensor
    rec: torch.Tensor
    S: int
    aug: Optional[torch.Tensor] = None
    photo: Optional[torch.Tensor] = None

    @property
    def shape(self) -> tuple:
        return (self.src.shape[0], self.S, self.S, 3)

    def to(self, dev, *a, **kw) -> '_SupportWindows':
        return _moved(self, dev)

    def stem_input(self, lut: torch.Tensor) -> tuple:
        """(the NHWC4 fp32 input of the stem, the masks uint8 [n,S,S]): crop, resize, pad and normalise in ONE launch,
        which makes the masks too; with ``aug`` the cut as bytes, the photometric pass where an instance has one, the
        gather."""
        if self.aug is None:
            return ops.support_from_source(self.src, self.msk, self.rec, lut, self.S)
        crop, msk = ops.support_from_source_u8(self.src, self.msk, self.rec, self.S)
        if self.photo is not None:                  # ([n,64]: one operator per instance; [n,P,64]: a chain of them)
            run = ops.photometric_u8 if self.photo.dim() == 2 else ops.photometric_chain_u8
            crop = run(crop.view(crop.shape[0], -1), self.photo).view(crop.shape)
        return ops.support_augment(crop, msk, self.aug, lut, self.S)


class _StemReady(NamedTuple):
    """An image batch that already is the NHWC4 fp32 input of the stem (``_SupportWindows.stem_input`` makes it together
    with the masks): ``_stem_input`` hands ``x`` through."""
    x: torch.Tensor

    @property
    def shape(self) -> tuple:
        return tuple(self.x.shape[:3]) + (3,)

    def to(self, dev, *a, **kw) -> '_StemReady':
        return self

    def stem_input(self, lut: torch.Tensor) -> torch.Tensor:
        return self.x


class _InputForm(NamedTuple):
    """The form in which one ``detect_device`` call brought its images: ``source``, the checked dict of
    ``FGN._source_query`` (None: ``qry_img`` is a tensor); ``spp_source``, the checked dict of ``FGN._source_supports``
    (None: ``spp_imgs`` is a tensor, or a support code stands in); ``at_source``, results at source size.  The one place
    that names the slot tensors these forms travel in - ``qry_src`` uint8 [B, slot] with ``qry_src_hw`` int32 [B,2],
    ``spp_src`` / ``spp_msk`` uint8 [B*N*K, slot] beside ``spp_rec`` - between ``_upload``, which fills them
    (``_upload_source`` / ``_upload_supports``), the static buffers of a captured graph and the carriers of the stem."""
    source: Optional[dict] = None
    spp_source: Optional[dict] = None
    at_source: bool = False

    def slots(self) -> dict:
        """name -> (rows, capacity) of the uint8 tensors whose rows have a configured capacity: a captured graph holds
        them at that size, a batch fills the fronts of their rows."""
        out = {}
        if self.source is not None:
            out['qry_src'] = (self.source['B'], self.source['capacity'])
        if self.spp_source is not None:
            out['spp_src'] = (self.spp_source['n'], self.spp_source['capacity'])
            out['spp_msk'] = (self.spp_source['n'], self.spp_source['mcapacity'])
        return out

    def key(self, ins: dict) -> tuple:
        """This form's part of a graph key, and the (name, shape, dtype) of every other tensor of ``ins``."""
        q, s = self.source, self.spp_source
        # source-size queries: the slot and the size they are resized to - NOT the source sizes, which the kernel
        # reads from ``qry_src_hw`` (the slot tensors are in ``ins`` only once they are uploaded: keyed here)
        # ... and whether the results are made at source size: another launch sequence (one batch-wide RLE launch
        # that reads ``qry_src_hw``); a graph captured without it keeps its key
        return (None if q is None else (q['B'], q['capacity'], q['hw']) + (('at_source',) if self.at_source else ()),) + \
            (() if s is None else     # supports from their sources: the window slots and S, no size of a batch
             (('spp_source', s['n'], s['capacity'], s['mcapacity'], s['S']),)) + \
            tuple((k, tuple(v.shape), v.dtype) for k, v in ins.items()
                  if v is not None and k not in ('qry_src', 'qry_src_hw', 'spp_src', 'spp_msk'))

    def query(self, t: dict):
        """The query of a dict of tensors (the uploaded ``ins``, or the static buffers of a graph) as ``_stem_input``
        takes it."""
        if self.source is None:
            return t.get('qry_img')
        return _QueryPixels(t['qry_src'], t['qry_src_hw'], *self.source['hw'])

    def supports(self, t: dict):
        """Likewise the supports as ``_support_front`` takes them."""
        if self.spp_source is None:
            return t.get('spp_imgs')
        return _SupportWindows(t['spp_src'], t['spp_msk'], t['spp_rec'], self.spp_source['S'])


class FGN(torch.nn.Module):
    """Fully Guided Network, inference path, on MI355X HIP kernels."""
    fp16_enabled = False
    subsampling_ratio = 16

    def __init__(self, n_ways: int, k_shots: int, backbone: Optional[dict] = None, rpn_head: Optional[dict] = None,
                 roi_head: Optional[dict] = None, train_cfg: Optional[dict] = None, test_cfg: Optional[dict] = None,
                 neck=None, pretrained=None, init_cfg=None, state_dict: Optional[dict] = None, seed: int = 0,
                 type: Optional[str] = None, **kwargs):
        super().__init__()
        if type not in (None, 'FGN'):
            raise ValueError(f'cannot build detector type {type!r}')
        self.n_ways, self.k_shots = int(n_ways), int(k_shots)
        self.cfg = normalise_config(self.n_ways, self.k_shots, backbone, rpn_head, roi_head, test_cfg, train_cfg)
        self.train_cfg = train_cfg
        self.test_cfg = self.cfg['test_cfg']
        # Region semantics of the mask paste (mmdet `_do_paste_mask`): 'cpu' = skip_empty=True, a mask is pasted inside the
        # integer-expanded box only - the CPU reference north_star names, this build's oracle and default; 'cuda' =
        # skip_empty=False, the grid spans the whole image - what the reference computes where it actually runs (cuda:0,
        # main.py:365).  Identical at the configured threshold 0.5 for boxes of positive width and height
        # (fgn_r50_c4_densecl.py:186: the value on the box edge is half the border pixel), up to box_w / 28 more pixels outside the box under 'cuda' below it.
        self.paste_semantics = 'cpu'
        if self.test_cfg['rcnn'].get('mask_thr_binary', 0.5) < 0.5:
            import warnings
            warnings.warn("mask_thr_binary < 0.5: mmdet's CPU and CUDA paste paths differ below 0.5 (skip_empty); this "
                          "detector follows the CPU path unless `paste_semantics = 'cuda'` is set (DESIGN.md section 2)",
                          stacklevel=2)
        self._sd = OrderedDict((k, self._canon(k, v)) for k, v in
                               (state_dict if state_dict is not None else init_state_dict(self.cfg, seed)).items())
        # mmcv `Pretrained` init_cfg of the backbone (fgn_r50_c4_densecl.py:39-41) / the deprecated `pretrained=` kwarg:
        # applied by init_weights(), as in the reference (main.py:431-434)
        ic = (backbone or {}).get('init_cfg') or init_cfg
        ic = ic[0] if isinstance(ic, (list, tuple)) and ic else ic
        self.backbone_pretrained = pretrained or (ic.get('checkpoint') if isinstance(ic, dict) and
                                                  ic.get('type') == 'Pretrained' else None) or None
        self._frozen_stages = int((backbone or {}).get('frozen_stages', 4)) if isinstance(backbone, dict) else 4
        self._packed_device = None
        self._PT = None                           # train-mode layers of the shared head (fgn_amd.train.pack_train)
        self.debug_trace: Optional[dict] = None   # set to {} to capture intermediates (tests)
        self.use_side_stream = True               # support branch on a second HIP stream
        self.use_graphs = False                   # replay a captured hipGraph per input geometry
        # exact overlap counts |d & g|, |d|, |g| of every detection with every ground-truth mask of its image, counted
        # on the device while the episode is in flight (result keys dt_gt_inter / dt_area / gt_area: the evaluator then
        # decodes no RLE); needs ``qry_isegmaps``.  False: nothing is launched, allocated or added
        self.match_on_device = False
        # the evaluator's greedy matching on the device as well: implies the counts above for the call;
        # ``detect_device`` runs ``ops.eval_match`` per image behind them and the result dicts gain ``dt_match_bbox``,
        # ``dt_match_segm`` (bit t = matched at ``eval_iou_thrs[t]``, -1 = beyond the evaluator's 100 per category),
        # ``eval_iou_thrs`` and ``gt_per_cat`` - all ``FSISEGEval`` needs besides scores and labels.  Off: nothing is
        # launched, allocated or added.
        self.evaluate_on_device = False
        self.eval_iou_thrs = (0.5,)         # 1..16 thresholds; COCO's ten: ``fsiseg_eval.COCO_IOU_THRS``
        self._use_winograd = ops.WINOGRAD_M       # Winograd form of the 3x3 / stride 1 convs: 4 = F(4x4,3x3), 2 = F(2x2,3x3), 0 = direct
        self.use_roi_commute = True               # shared_head conv1 on the feature map, RoIAlign after (set before first use)
        # query + support maps through SHARED backbone launches (1x1 / stride 1 convolutions and the grouped Winograd GEMM
        # over all rows of both; frozen-BN bottleneck backbones): half the launches of the two passes, no support-only
        # split-K.  Round 2 measured this 5 % slower with one episode in flight (the support stream filled the query
        # branch's idle phases); with two episodes in flight the other episode does that, and it is 7 % faster
        # (same-box A/B, r03: 6.07 -> 5.72 ms).  Results differ from the separate passes in the last bits only
        # (split-K plans and Winograd-vs-direct choices depend on the row count).
        self.use_merged_backbone = True
        # the support RoIs ride through the shared head in the box head's RoI batch (same weights; eval-mode BatchNorm is
        # per sample): the ~30 small launches of count_spp's own shared-head pass (9 RoIs, 441 rows: three direct-form
        # 3x3 convolutions at 0.08 of the MFMA peak while they queue behind the persistent GEMMs, r03 kernel stats)
        # disappear into 3 % more rows of the 300-RoI launches.  Step time equal within run-to-run noise (same-box A/B,
        # r04: B = 1 189.9-191.3 vs 188.6-190.9 img/s, B = 4 211.1-211.8 vs 209.2-211.0, B = 8 214.6 vs 215.5): on since
        # round 4 for the launch count.  False = the separate pass, byte-identical to `encode_supports`.
        self.use_merged_support_head = True
        self.transfer_mode = 0                    # 0: upload + copy stream per caller; 1 / 2: see transfer_stream()
        # one device-to-host copy per batch (every output lands in one `_ResultRecord`) and, under graph replay with the
        # transfers on the caller stream, host inputs copied straight into the graph's static buffers (round 5: 15 -> 6
        # small copies per episode on the caller stream); False = the per-field copies of rounds 1-4 (A/B knob)
        self.use_packed_transfers = True
        self.stamp_capacity = 0                   # > 0: captured graphs carry launch records of the dominant kernel (ops.read_stamps)
        self._graphs: dict = {}
        # bytes per image of the static source slot of a captured graph (``qry_resize_to`` under ``use_graphs``): the
        # graph key holds this size, not the source sizes, so every source that fits replays one graph
        self.query_source_capacity = 3 * 2_000_000
        # the same for supports cut from their source images (``spp_crop_to`` under ``use_graphs``): bytes per INSTANCE of
        # the image-window slot (the mask-window slot is a third of it); the default holds a 640 x 640 window
        self.support_source_capacity = 3 * 640 * 640
        self.input_lut: Optional[np.ndarray] = None   # [3,256] fp32 normalisation table of uint8 images (set_input_norm)
        self._input_lut_dev = None                # (device, its copy there)
        self._streams: dict = {}                  # (role, caller stream) -> HIP stream: 'side', 'copy', 'upload'
        self._pinned: dict = {}                   # (batch, max_det, byte cap) -> list of pinned host slots

    def _skip_empty(self) -> bool:
        if self.paste_semantics not in ('cpu', 'cuda'):
            raise ValueError(f"paste_semantics must be 'cpu' or 'cuda', got {self.paste_semantics!r}")
        return self.paste_semantics == 'cpu'

    @property
    def use_winograd(self) -> int:
        return self._use_winograd

    @use_winograd.setter
    def use_winograd(self, on) -> None:
        """False / 0: direct implicit GEMM for every 3x3; True: the default Winograd form (F(4x4,3x3)); 2 or 4: that
        output tile edge."""
        m = ops.WINOGRAD_M if on is True else int(on)
        if m not in (0, 2, 4):
            raise ValueError('use_winograd: False, True, 2 or 4')
        if m != self._use_winograd:               # the packed layers (and any captured graph) depend on it
            self._use_winograd = m
            self._packed_device = None
            self._PT = None
            self._graphs = {}

    @classmethod
    def from_config(cls, model_cfg: dict, **kw) -> 'FGN':
        """``build_detector(cfg.model, ...)`` equivalent (main.py:390-394)."""
        model_cfg = copy.deepcopy(dict(model_cfg))
        model_cfg.pop('type', None)
        model_cfg.update(kw)
        return cls(**model_cfg)

    # --- weights --------------------------------------------------------------------------
    def _trainer_alive(self):
        ref = getattr(self, '_trainer', None)
        return ref() if ref is not None else None

    def _source_sd(self) -> dict:
        """The weights every (re-)pack starts from: the state dict, overlaid with the device-resident master weights
        and running statistics of a live ``fgn_amd.train.Trainer`` - so a re-pack after training steps (device change,
        ``use_winograd`` setter, ``_packed_device`` reset) never falls back to the initial heads."""
        tr = self._trainer_alive()
        if tr is None:
            return self._sd
        sd = OrderedDict(self._sd)
        sd.update(tr.W)
        sd.update(tr.buffers)
        return sd

    def state_dict(self, *a, **k):
        tr = self._trainer_alive()
        return OrderedDict(self._sd) if tr is None else OrderedDict(tr.state_dict())

    @staticmethod
    def _canon(name: str, v: torch.Tensor) -> torch.Tensor:
        return v.detach().cpu() if name.endswith('num_batches_tracked') else v.detach().float().cpu()

    @property
    def backbone(self):
        """What main.py:402-405 reads off ``model.backbone`` right after ``build_detector``: ``frozen_stages`` (from the
        reference's config dict; 4 = the DenseCL configuration, -1 = from scratch), the list of stage names it shortens
        to drop res5 (this detector is C4 by construction: three stages), and ``eval()`` (BatchNorm is folded from the
        running statistics at pack time: there is no train-mode backbone to switch)."""
        from types import SimpleNamespace
        ns = SimpleNamespace(frozen_stages=self._frozen_stages, norm_eval=bool(self.cfg['backbone'].get('norm_eval', True)),
                             res_layers=[f'layer{i + 1}' for i in range(len(self.cfg['backbone']['stage_blocks']) + 1)])
        ns.eval = lambda: ns
        ns.train = lambda mode=True: ns
        return ns

    def init_weights(self) -> None:
        """mmcv ``BaseModule.init_weights`` as far as this path needs it: the backbone's ``Pretrained`` init_cfg
        (fgn_r50_c4_densecl.py:39-41; main.py:431-434).  Without one the seeded initialisation stands."""
        if self.backbone_pretrained:
            self.load_backbone_pretrained(self.backbone_pretrained)

    def load_backbone_pretrained(self, ckpt) -> dict:
        """Load a backbone-only checkpoint (path, or state dict with un-prefixed torchvision / mmcv ResNet keys) into
        ``backbone.*`` only, non-strict like mmcv's ``load_checkpoint(backbone, ..., strict=False)``: entries the C4
        backbone does not have (``layer4.*``, ``fc.*``) are reported as unexpected, absent ones as missing (the
        optional ``num_batches_tracked`` buffers aside).  Heads keep their weights."""
        src = backbone_state_from_pretrained(ckpt)
        own = [k for k in self._sd if k.startswith('backbone.')]
        picked = {k: src[k] for k in own if k in src}
        for k, v in picked.items():
            if tuple(v.shape) != tuple(self._sd[k].shape):
                raise ValueError(f'shape mismatch for {k}: {tuple(v.shape)} vs {tuple(self._sd[k].shape)}')
        report = dict(loaded=len(picked),
                      missing=[k for k in own if k not in src and not k.endswith('num_batches_tracked')],
                      unexpected=[k for k in src if k not in self._sd])
        if not picked:
            raise KeyError('no backbone tensor found in the checkpoint (expected keys like conv1.weight, layer1.0.conv1.weight)')
        self.load_state_dict(picked, strict=False)
        return report

    def load_state_dict(self, state_dict, strict: bool = True):
        sd = state_dict.get('state_dict', state_dict)
        missing = [k for k in self._sd if k not in sd and not k.endswith('num_batches_tracked')]
        if strict and missing:
            raise KeyError(f'missing keys in state_dict: {missing[:5]} ...')
        for k in self._sd:
            if k in sd:
                if tuple(sd[k].shape) != tuple(self._sd[k].shape):
                    raise ValueError(f'shape mismatch for {k}: {tuple(sd[k].shape)} vs {tuple(self._sd[k].shape)}')
                self._sd[k] = self._canon(k, sd[k])
        self._packed_device = None
        self._PT = None
        self._graphs = {}
        tr = self._trainer_alive()
        if tr is not None:              # a live trainer adopts the loaded weights (its Adagrad sums are kept)
            tr.adopt(self._sd)

    def _pack(self, device):
        """Fold BN, re-layout weights for the kernels and move them to ``device``."""
        sd, cfg = self._source_sd(), self.cfg
        eps = cfg['backbone']['bn_eps']
        P = {}
        bb = cfg['backbone']
        gn = bb.get('norm', 'BN') == 'GN'
        bnp = lambda name: {k: sd[f'{name}.{k}'] for k in ('weight', 'bias', 'running_mean', 'running_var')}
        # stem: list of (conv, GroupNorm params or None); BatchNorm(eval) folds into the conv epilogue
        if bb.get('deep_stem'):
            P['stem'] = []
            for i, stride in enumerate((2, 1, 1)):
                w, nm = sd[f'backbone.stem.{3 * i}.weight'], f'backbone.stem.{3 * i + 1}'
                kw = dict(stride=stride, pad=1, pad_cin_to=4 if i == 0 else None)
                if gn:
                    P['stem'].append((ops.pack_conv(w, **kw), [sd[nm + '.weight'].clone(), sd[nm + '.bias'].clone()]))
                else:
                    P['stem'].append((ops.pack_conv(w, bn=bnp(nm), relu=True, eps=eps, **kw), None))
        elif gn:
            P['stem'] = [(ops.pack_conv(sd['backbone.conv1.weight'], stride=2, pad=3, pad_cin_to=4),
                          [sd['backbone.gn1.weight'].clone(), sd['backbone.gn1.bias'].clone()])]
        else:
            P['stem'] = [(ops.pack_conv(sd['backbone.conv1.weight'], bn=bnp('backbone.bn1'), stride=2, pad=3,
                                        relu=True, eps=eps, pad_cin_to=4), None)]
        P['stages'] = []
        for li, (nblk, stride) in enumerate(zip(bb['stage_blocks'], bb['strides'])):
            P['stages'].append([
                _BottleneckGN(sd, f'backbone.layer{li + 1}.{b}', stride if b == 0 else 1, bb.get('gn_groups', 32),
                              eps, bb.get('avg_down', False)) if gn else
                (_BasicBlock if bb.get('block', 'bottleneck') == 'basic' else _Bottleneck)(
                    sd, f'backbone.layer{li + 1}.{b}', stride if b == 0 else 1, eps, winograd=self.use_winograd)
                for b in range(nblk)])
        P.update(self._pack_heads(sd))
        P.update(self._pack_shared(sd))
        rp = cfg['rpn_head']
        P['anchors'] = torch.from_numpy(ops.base_anchors(rp['anchor_scales'], rp['anchor_ratios'],
                                                         rp['anchor_stride']))

        def mv(o):
            if isinstance(o, torch.Tensor):
                return o.float().contiguous().to(device)
            if isinstance(o, (ops.ConvLayer, ops.WinogradLayer, ops.DualConvLayer)):
                return o.to(device)
            if isinstance(o, (_Bottleneck, _BasicBlock)):
                for l in o.layers():
                    l.to(device)
                return o
            if isinstance(o, _BottleneckGN):
                return o.to(device)
            if isinstance(o, (list, tuple)):
                return [mv(x) for x in o]
            return o
        self._P = {k: mv(v) for k, v in P.items()}
        self._packed_device = torch.device(device)
        self._shared_dirty = None
        if self._trainer_alive() is not None:      # the train-mode layers follow the same weights
            self._PT = None

    def _head_math(self):
        """Arithmetic of the trainable layers' GEMMs: f32 MFMA while a Trainer rewrites their weights every step
        (``ops.gemm_math``), the build's default otherwise."""
        return 'f32' if self._trainer_alive() is not None else None

    def _pack_shared(self, sd) -> dict:
        with ops.gemm_math(self._head_math()):
            return self._pack_shared_impl(sd)

    def _pack_heads(self, sd) -> dict:
        with ops.gemm_math(self._head_math()):
            return self._pack_heads_impl(sd)

    def _pack_shared_impl(self, sd) -> dict:
        """The shared head for INFERENCE (BatchNorm in eval mode, folded into the conv epilogues) from torch-layout
        weights and running statistics ``sd`` (CPU state dict, or a Trainer's device-resident masters + buffers)."""
        cfg = self.cfg
        eps = cfg['backbone']['bn_eps']
        P = {}
        P['shared'] = [_Bottleneck(sd, f'roi_head.shared_head.{b}', 1, eps, winograd=self.use_winograd)
                       for b in range(cfg['roi_head']['shared_head']['num_blocks'])]
        # conv1 of the first shared_head block with its BN scale folded and no shift / ReLU: applied to the C4 map
        # (RoIAlign commutes with it); the shift is added after the pooling
        c1 = P['shared'][0].conv1
        P['sh0_lin'] = ops.ConvLayer(c1.w.clone(), None if c1.scale is None else c1.scale.clone(), None, c1.cin,
                                     c1.cout, c1.cout_pad, c1.kh, c1.kw, c1.stride, c1.pad, False,
                                     None if c1.w3 is None else c1.w3.clone(), None if c1.wh is None else c1.wh.clone()) \
            if self.use_roi_commute else None
        P['sh0_shift'] = c1.shift.clone() if (self.use_roi_commute and c1.shift is not None) else None
        return P

    def _pack_heads_impl(self, sd) -> dict:
        """The packed AG-RPN / relation / box / mask head layers from torch-layout weights ``sd`` (CPU tensors of the
        state dict, or the device-resident master weights of ``fgn_amd.train.Trainer``: packing is torch ops only)."""
        cfg = self.cfg
        P = {}
        P['rpn_conv'] = ops.pack_conv(sd['rpn_head.rpn_conv.weight'], bias=sd['rpn_head.rpn_conv.bias'], pad=1,
                                      relu=True)
        wr = sd['rpn_head.rpn_conv.weight']
        P['rpn_conv_wg'] = ops.pack_winograd(wr, bias=sd['rpn_head.rpn_conv.bias'], relu=True, m=self.use_winograd) \
            if self.use_winograd and wr.shape[1] % 32 == 0 and wr.shape[0] % 4 == 0 else None
        # objectness and delta 1x1 convs fused into one launch: channels [0,A) | [A,5A)
        # (zero rows pad the 5A = 75 channels to a multiple of 4: 16-byte epilogue stores and split-K become
        # available to the launch; rpn_merge reads the first 5A channels of each pixel)
        wh = torch.cat([sd['rpn_head.rpn_cls.weight'], sd['rpn_head.rpn_reg.weight']], 0)
        bh = torch.cat([sd['rpn_head.rpn_cls.bias'], sd['rpn_head.rpn_reg.bias']], 0)
        padc = (-wh.shape[0]) % 4
        if padc:
            wh = torch.cat([wh, wh.new_zeros((padc,) + tuple(wh.shape[1:]))], 0)
            bh = torch.cat([bh, bh.new_zeros(padc)], 0)
        P['rpn_head'] = ops.pack_conv(wh, bias=bh)
        # relation conv split along its input channels: [Wq | Ws] (fgn_roi_head.py:270)
        wrel = sd['roi_head.cls_reg_shared_conv.weight']
        c = wrel.shape[1] // 2
        P['rel_q'] = ops.pack_conv(wrel[:, :c].contiguous())
        P['rel_s'] = ops.pack_conv(wrel[:, c:].contiguous(), bias=sd['roi_head.cls_reg_shared_conv.bias'])
        P['gn_w'] = sd['roi_head.cls_reg_shared_conv_norm.weight'].clone()
        P['gn_b'] = sd['roi_head.cls_reg_shared_conv_norm.bias'].clone()
        P['fc_w'] = torch.cat([sd['roi_head.bbox_head.fc_cls.weight'], sd['roi_head.bbox_head.fc_reg.weight']], 0)
        P['fc_b'] = torch.cat([sd['roi_head.bbox_head.fc_cls.bias'], sd['roi_head.bbox_head.fc_reg.bias']], 0)
        mh = cfg['roi_head']['mask_head']
        P['mask_convs'] = [ops.pack_conv(sd[f'roi_head.mask_head.convs.{i}.conv.weight'],
                                         bias=sd[f'roi_head.mask_head.convs.{i}.conv.bias'], pad=1, relu=True)
                           for i in range(mh['num_convs'])]
        P['mask_convs_wg'] = [
            ops.pack_winograd(sd[f'roi_head.mask_head.convs.{i}.conv.weight'],
                              bias=sd[f'roi_head.mask_head.convs.{i}.conv.bias'], relu=True, m=self.use_winograd)
            if self.use_winograd and sd[f'roi_head.mask_head.convs.{i}.conv.weight'].shape[1] % 32 == 0 and
            sd[f'roi_head.mask_head.convs.{i}.conv.weight'].shape[0] % 4 == 0 else None
            for i in range(mh['num_convs'])]
        # ConvTranspose2d(k=2,s=2) [Cin,Cout,2,2] -> 1x1 conv with 4*Cout outputs, n=(dy*2+dx)*Cout+co
        wt = sd['roi_head.mask_head.upsample.weight']
        cin_u, cout_u = wt.shape[:2]
        w4 = wt.permute(2, 3, 1, 0).reshape(4 * cout_u, cin_u, 1, 1).contiguous()
        P['upsample'] = ops.pack_conv(w4, bias=sd['roi_head.mask_head.upsample.bias'].repeat(4), relu=True)
        P['logit_w'] = sd['roi_head.mask_head.conv_logits.weight'].reshape(-1).clone()
        # a float for host-resident weights; the device-resident master weights of a Trainer stay on the device (the
        # kernel reads the bias through a pointer: no host synchronisation at the end of every training step)
        lb = sd['roi_head.mask_head.conv_logits.bias']
        P['logit_b'] = lb.reshape(-1)[:1].float().contiguous().clone() if lb.is_cuda else float(lb[0])
        return P

    def _repack_heads_(self, sd) -> None:
        """``_pack_heads`` of updated DEVICE weights into the layers ``self._P`` already holds (same shapes): one strided
        copy per convolution, one kernel per Winograd layer, no allocation - the re-pack between two training steps
        (round 4: 2.5 ms of ~150 torch kernels -> a few dozen launches).  Same values as a fresh ``_pack_heads``."""
        P = self._P
        ops.repack_conv_(P['rpn_conv'], sd['rpn_head.rpn_conv.weight'], sd['rpn_head.rpn_conv.bias'])
        if P['rpn_conv_wg'] is not None:
            ops.repack_winograd_(P['rpn_conv_wg'], sd['rpn_head.rpn_conv.weight'], sd['rpn_head.rpn_conv.bias'])
        # fused objectness + delta 1x1 conv: channels [0, A) | [A, 5A) (+ zero rows up to a multiple of 4)
        h = P['rpn_head']
        a = sd['rpn_head.rpn_cls.weight'].shape[0]
        n = a + sd['rpn_head.rpn_reg.weight'].shape[0]
        h.w[:a, :h.cin].copy_(sd['rpn_head.rpn_cls.weight'].reshape(a, h.cin))
        h.w[a:n, :h.cin].copy_(sd['rpn_head.rpn_reg.weight'].reshape(n - a, h.cin))
        h.shift[:a].copy_(sd['rpn_head.rpn_cls.bias'])
        h.shift[a:n].copy_(sd['rpn_head.rpn_reg.bias'])
        wrel = sd['roi_head.cls_reg_shared_conv.weight']
        c = wrel.shape[1] // 2
        P['rel_q'].w[:wrel.shape[0], :c].copy_(wrel[:, :c, 0, 0])
        P['rel_s'].w[:wrel.shape[0], :c].copy_(wrel[:, c:, 0, 0])
        P['rel_s'].shift.copy_(sd['roi_head.cls_reg_shared_conv.bias'])
        P['gn_w'].copy_(sd['roi_head.cls_reg_shared_conv_norm.weight'])
        P['gn_b'].copy_(sd['roi_head.cls_reg_shared_conv_norm.bias'])
        nc = sd['roi_head.bbox_head.fc_cls.weight'].shape[0]
        P['fc_w'][:nc].copy_(sd['roi_head.bbox_head.fc_cls.weight'])
        P['fc_w'][nc:].copy_(sd['roi_head.bbox_head.fc_reg.weight'])
        P['fc_b'][:nc].copy_(sd['roi_head.bbox_head.fc_cls.bias'])
        P['fc_b'][nc:].copy_(sd['roi_head.bbox_head.fc_reg.bias'])
        for i, (layer, wg) in enumerate(zip(P['mask_convs'], P['mask_convs_wg'])):
            w, b = sd[f'roi_head.mask_head.convs.{i}.conv.weight'], sd[f'roi_head.mask_head.convs.{i}.conv.bias']
            ops.repack_conv_(layer, w, b)
            if wg is not None:
                ops.repack_winograd_(wg, w, b)
        # ConvTranspose2d(k=2,s=2) [Cin,Cout,2,2] -> 1x1 conv with 4*Cout outputs, n=(dy*2+dx)*Cout+co
        wt = sd['roi_head.mask_head.upsample.weight']
        cin_u, cout_u = wt.shape[:2]
        up = P['upsample']
        up.w[:4 * cout_u].view(2, 2, cout_u, up.w.shape[1])[..., :cin_u].copy_(wt.permute(2, 3, 1, 0))
        up.shift.view(4, cout_u).copy_(sd['roi_head.mask_head.upsample.bias'].expand(4, cout_u))
        P['logit_w'].copy_(sd['roi_head.mask_head.conv_logits.weight'].reshape(-1))
        P['logit_b'].copy_(sd['roi_head.mask_head.conv_logits.bias'].reshape(-1)[:1])

    # --- input images ---------------------------------------------------------------------
    def set_input_norm(self, mean=None, std=None, scale: float = 255.0, lut=None) -> None:
        """Accept decoded images: with a table set, every ``torch.uint8`` image tensor is taken as channels-last pixels
        (``qry_img`` [B,H,W,3], ``spp_imgs`` [B,N*K,S,S,3] or [N*K,S,S,3]) and normalised on the device,
        ``(v / scale - mean[c]) / std[c]`` through a per-channel table of the 256 byte values built here in the data
        loader's float32 arithmetic (``ops.input_lut``) - the same bytes as the host-normalised float NCHW image, without
        the host arithmetic and with a quarter of the upload.  Float tensors keep going the NCHW way, per tensor.
        ``lut``: a ready [3,256] table instead of mean / std.  No arguments: back to float input only (a uint8 tensor is
        then cast as it is, as before)."""
        if lut is not None:
            if mean is not None or std is not None:
                raise ValueError('set_input_norm: give mean and std, or lut')
            table = np.ascontiguousarray(np.asarray(lut, np.float32))
            if table.shape != (3, 256):
                raise ValueError(f'set_input_norm: lut must be [3,256], got {list(table.shape)}')
        elif mean is not None:
            if std is None:
                raise ValueError('set_input_norm: mean needs std')
            table = ops.input_lut(mean, std, scale)
        elif std is not None:
            raise ValueError('set_input_norm: std needs mean')
        else:
            table = None
        self.input_lut = table
        self._input_lut_dev = None
        self._graphs = {}               # the table's device address is an argument of the captured launches

    def _lut_on(self, dev) -> torch.Tensor:
        if self._input_lut_dev is None or self._input_lut_dev[0] != dev:
            self._input_lut_dev = (dev, torch.from_numpy(self.input_lut).to(dev))
        return self._input_lut_dev[1]

    def _image_dims(self, img: Union[torch.Tensor, '_QueryPixels'], what: str, lead=(1,)) -> tuple:
        """(leading dimensions, H, W) of an image tensor as given: channels-last pixels when it is uint8 and a table is
        set (``set_input_norm``), NCHW otherwise; source-size pixels (``_QueryPixels``) count with the size they are
        resized to.  ``lead``: the numbers of leading dimensions allowed."""
        if not isinstance(img, torch.Tensor):
            return img.dims
        if self.input_lut is not None and img.dtype == torch.uint8:
            if img.dim() - 3 not in lead or img.shape[-1] != 3:
                raise ValueError(f'{what}: with set_input_norm in effect a uint8 image tensor is channels-last pixels '
                                 f'[..,H,W,3] behind {" or ".join(str(n) for n in lead)} leading dimension(s), got '
                                 f'{list(img.shape)}')
            return tuple(img.shape[:-3]), int(img.shape[-3]), int(img.shape[-2])
        return tuple(img.shape[:-3]), int(img.shape[-2]), int(img.shape[-1])

    def _stem_input(self, img: Union[torch.Tensor, '_QueryPixels', '_StemReady']) -> torch.Tensor:
        """Image batch as given (host or device) -> the NHWC4 fp32 input of the stem on the current device: uint8 pixels
        [n,H,W,3] through the normalisation table, source-size pixels (``_QueryPixels``) resized and normalised in one
        kernel, a ready stem input (``_StemReady``: supports cut from their sources) as it is, anything else cast to fp32
        NCHW [n,3,H,W] and re-laid."""
        dev = torch.device('cuda', torch.cuda.current_device())
        if not isinstance(img, torch.Tensor):       # (a carrier answers for itself)
            return img.to(dev).stem_input(self._lut_on(dev))
        if self.input_lut is not None and img.dtype == torch.uint8:
            self._image_dims(img, 'image')
            return ops.u8hwc3_to_nhwc4(img.to(dev, non_blocking=True).contiguous(), self._lut_on(dev))
        return ops.nchw3_to_nhwc4(img.to(dev, torch.float32, non_blocking=True).contiguous())

    def _source_query(self, qry_img, qry_resize_to, img_shape, qry_isegmaps=None, graphed: bool = False) -> dict:
        """The contract of ``qry_resize_to`` (host only, nothing is queued): ``qry_img`` is a uint8 tensor [B,h,w,3] or
        a list of B uint8 tensors [h_i,w_i,3], a table is set, (H, W) comes as a pair or as a [B,2] tensor of equal
        rows, ``img_shape`` (default (H, W, 3) per image) agrees with it, the masks are at their image's source size and
        every image fits the slot.  -> B, (H, W), the images as flat byte tensors, their sizes, the slot size in bytes
        per image and ``img_shape``."""
        rt = _host(qry_resize_to)
        ok = rt.dtype.kind in 'iuf' and (rt.shape == (2,) or (rt.ndim == 2 and rt.shape[1] == 2 and rt.shape[0] >= 1))
        if ok:
            rt = rt.reshape(-1, 2)
            ok = bool(np.all(rt == np.floor(rt)) and np.all(rt == rt[:1]))
        if not ok:
            raise ValueError(f'qry_resize_to must be (H, W) or a [B,2] tensor of equal rows, got {qry_resize_to!r}')
        H, W = int(rt[0, 0]), int(rt[0, 1])
        if not (1 <= H <= ops.RESIZE_MAX_DIM and 1 <= W <= ops.RESIZE_MAX_DIM):
            raise ValueError(f'qry_resize_to: sizes must be within 1..{ops.RESIZE_MAX_DIM}, got {(H, W)}')
        if self.input_lut is None:
            raise ValueError('qry_resize_to needs the normalisation table: call set_input_norm first')
        imgs = list(qry_img) if isinstance(qry_img, (list, tuple)) else qry_img
        if isinstance(imgs, torch.Tensor):
            if imgs.dim() != 4:
                raise ValueError(f'qry_img: with qry_resize_to, a uint8 tensor [B,h,w,3] or a list of [h,w,3] tensors, '
                                 f'got {list(imgs.shape)}')
            imgs = list(imgs.unbind(0))
        for im in imgs:
            if not isinstance(im, torch.Tensor) or im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3:
                what = f'{im.dtype} {list(im.shape)}' if isinstance(im, torch.Tensor) else type(im).__name__
                raise ValueError(f'qry_img: with qry_resize_to every image is channels-last uint8 pixels [h,w,3], got {what}')
            if not (1 <= im.shape[0] <= ops.RESIZE_MAX_DIM and 1 <= im.shape[1] <= ops.RESIZE_MAX_DIM):
                raise ValueError(f'qry_img: source sizes must be within 1..{ops.RESIZE_MAX_DIM}, got {list(im.shape)}')
        B = len(imgs)
        if len(rt) not in (1, B):
            raise ValueError(f'qry_resize_to has {len(rt)} rows for {B} images')
        if img_shape is None:
            img_shape = np.tile(np.array([H, W, 3], np.int32), (B, 1))
        elif len(img_shape) != B or any(int(sh[0]) != H or int(sh[1]) != W for sh in img_shape):
            raise ValueError(f'img_shape {[tuple(int(v) for v in sh) for sh in img_shape]} disagrees with '
                             f'qry_resize_to {(H, W)}')
        sizes = [(int(im.shape[0]), int(im.shape[1])) for im in imgs]
        if qry_isegmaps is not None:
            if len(qry_isegmaps) != B:
                raise ValueError(f'qry_isegmaps has {len(qry_isegmaps)} entries for {B} images')
            for i, (g, hw) in enumerate(zip(qry_isegmaps, sizes)):
                g = maskforms.checked(g, hw, f'qry_isegmaps[{i}]')     # (a carrier of ``_gt_entries`` passes by its shape)
                if len(g.shape) != 3 or (int(g.shape[1]), int(g.shape[2])) != hw:
                    raise ValueError(f'qry_isegmaps: with qry_resize_to the masks are at source size {hw}, got '
                                     f'{list(g.shape)}')
        need = max((3 * h * w for h, w in sizes), default=0)
        capacity = need
        if graphed:
            capacity = int(self.query_source_capacity)
            if need > capacity:
                raise ValueError(f'a query image of {need} bytes exceeds FGN.query_source_capacity = {capacity}: raise '
                                 f'the attribute (the static source slot of the captured graph)')
        return dict(B=B, hw=(H, W), flats=[im.contiguous().reshape(-1) for im in imgs], sizes=sizes, need=need,
                    capacity=capacity, img_shape=img_shape)

    def _gt_sizes(self, qry_img, img_shape, qry_resize_to):
        """The (h, w) the ground truth of every image is given at - its image's source size with ``qry_resize_to`` (the
        setting, or the dict of ``_source_query``), else the network size: ``img_shape``, or without it the size of the
        ``qry_img`` tensor itself - or None where the images do not say (they are refused next)."""
        if isinstance(qry_resize_to, dict):
            return qry_resize_to['sizes']
        if qry_resize_to is None:
            if img_shape is not None:
                return [(int(s[0]), int(s[1])) for s in img_shape]
            if not isinstance(qry_img, torch.Tensor) or qry_img.dim() != 4:
                return None
            try:
                (b,), h, w = self._image_dims(qry_img, 'qry_img')
            except ValueError:
                return None
            return [(h, w)] * b
        imgs = list(qry_img) if isinstance(qry_img, (list, tuple, torch.Tensor)) else []
        if not imgs or any(not isinstance(im, torch.Tensor) or im.dim() != 3 for im in imgs):
            return None
        return [(int(im.shape[0]), int(im.shape[1])) for im in imgs]

    def _gt_images(self, qry_img, qry_resize_to):
        """The images a box + colour entry is derived from, one [h,w,3] uint8 tensor per image, in the frame
        ``_gt_sizes`` names - the source images with ``qry_resize_to``, else the uint8 ``qry_img`` under a table - or None
        where the query is not bytes."""
        if isinstance(qry_resize_to, dict):
            return [f.view(h, w, 3) for f, (h, w) in zip(qry_resize_to['flats'], qry_resize_to['sizes'])]
        imgs = qry_img
        if qry_resize_to is None and (not isinstance(imgs, torch.Tensor) or imgs.dim() != 4 or self.input_lut is None):
            return None
        imgs = list(imgs) if isinstance(imgs, (list, tuple, torch.Tensor)) else []
        if not imgs or any(not isinstance(im, torch.Tensor) or im.dtype != torch.uint8 or im.dim() != 3 or
                           im.shape[2] != 3 for im in imgs):
            return None
        return imgs

    def _gt_front(self, qry_isegmaps, qry_img, img_shape, qry_resize_to):
        """``_gt_entries`` with the sizes and images of this call."""
        if qry_isegmaps is None or not isinstance(qry_isegmaps, (list, tuple)) or \
                not any(isinstance(g, (list, tuple)) or maskforms.form_of(g) is not None for g in qry_isegmaps):
            return qry_isegmaps
        return _gt_entries(qry_isegmaps, self._gt_sizes(qry_img, img_shape, qry_resize_to),
                           self._gt_images(qry_img, qry_resize_to))

    @staticmethod
    def _color_on_device(entries: list, slot: torch.Tensor) -> list:
        """The box + colour entries of ``entries`` (``ColorMasks``, entry b reading image b) made into dense uint8 masks
        [n_b,h_b,w_b] on the device from ``slot`` - uint8 [B, bytes], image b as [h_b,w_b,3] at the front of row b, AS
        UPLOADED - in ONE launch on the current stream, which is the stream that carried those bytes up (DESIGN
        4.4.11); every other entry stays as it is.  Without a colour entry nothing is called."""
        colour = [maskforms.form_of(g) is maskforms.COLOR for g in entries or ()]
        if not any(colour):
            return entries
        made = iter(ops.color_masks(slot, [(b, g) for b, g in enumerate(entries) if colour[b]]))
        return [next(made) if c else g for g, c in zip(entries, colour)]

    @staticmethod
    def _augment_plans(qry_augment, qry_bboxes, rs: dict) -> tuple:
        """The contract of ``qry_augment`` (host only, nothing is queued): [B,8] finite rows of
        ``fewshot_ds.AUG_PARAMS`` with flip, border and channel order inside their sets and coefficients inside the bounds
        of the integer rule.  -> (records int32 [B,16], the boxes at the network size): per image
        ``fewshot_ds.augment_plan`` - the boxes through the forward matrix, or, where a box leaves the image, the neutral
        record and the plain boxes (the fallback of base_fst.py:751-768)."""
        from . import fewshot_ds as fd
        rows = _number_rows(qry_augment, ((rs['B'], len(fd.AUG_PARAMS)),),
                            f'qry_augment must be [B,{len(fd.AUG_PARAMS)}] numbers {fd.AUG_PARAMS} for {rs["B"]} images')
        if qry_bboxes is None or len(qry_bboxes) != rs['B']:
            raise ValueError(f'qry_augment: qry_bboxes must hold the boxes of {rs["B"]} images')
        recs, boxes = [], []
        for row, b, hw in zip(rows, qry_bboxes, rs['sizes']):
            as_tensor = isinstance(b, torch.Tensor)
            rec, nb = fd.augment_plan(row, _host(b), hw, rs['hw'])
            recs.append(rec)
            boxes.append(torch.from_numpy(nb) if as_tensor else nb)
        return torch.from_numpy(np.stack(recs)), boxes

    @staticmethod
    def _photometric_records(qry_photometric, rs: dict, qry_augment=None, aug_recs=None):
        """The contract of ``qry_photometric`` (host only, nothing is queued): [B,3] finite rows of
        ``fewshot_ds.PHOTO_PARAMS`` with operator, amount and seed inside their sets and a blur radius of at most 16 source
        pixels.  -> records int32 [B,64] (``fewshot_ds.query_photometric_record``), or None when every row is neutral.
        An image whose geometric row fell back to the plain sample (``aug_recs``: a neutral record for a row that is
        not) gets the neutral record here too: ``bad_augment`` drops both halves (base_fst.py:751-768)."""
        from . import fewshot_ds as fd
        rows = _number_rows(qry_photometric, ((rs['B'], len(fd.PHOTO_PARAMS)),),
                            f'qry_photometric must be [B,{len(fd.PHOTO_PARAMS)}] numbers {fd.PHOTO_PARAMS} for '
                            f'{rs["B"]} images')
        recs = np.stack([fd.query_photometric_record(row, hw, rs['hw']) for row, hw in zip(rows, rs['sizes'])])
        if qry_augment is not None:
            for i, (g, hw) in enumerate(zip(_host(qry_augment), rs['sizes'])):
                if not fd.augment_is_neutral(fd.check_augment_params(g)) and not aug_recs[i, 2:6].any():
                    recs[i] = fd.query_photometric_record(None, hw, rs['hw'])
        return torch.from_numpy(recs) if recs[:, 2].any() else None

    @staticmethod
    def _chain_launch(recs: np.ndarray):
        """Compacted chain records int32 [n,3,64] (``fewshot_ds.photometric_chain_records``) -> what is launched: None
        where no image has an active operator; int32 [n,64], the records of the single-operator launch
        (``ops.photometric_u8``), where every image has at most one; else int32 [n,P,64], P the longest chain, for
        ``ops.photometric_chain_u8``."""
        depth = int((recs[:, :, 2] != 0).sum(1).max()) if len(recs) else 0
        if depth == 0:
            return None
        return torch.from_numpy(np.ascontiguousarray(recs[:, 0] if depth == 1 else recs[:, :depth]))

    @staticmethod
    def _photometric_chain_records(qry_photometric_chain, rs: dict, qry_augment=None, aug_recs=None):
        """The contract of ``qry_photometric_chain`` (host only, nothing is queued): [B,P,3] finite rows of
        ``fewshot_ds.PHOTO_PARAMS``, P in 1..3, each inside the sets of ``qry_photometric`` and of the form "point
        operators, then at most one blur" (``fewshot_ds.check_photometric_chain``).  -> ``_chain_launch`` of the compacted
        records; an image whose geometric row fell back gets the neutral chain, as in ``_photometric_records``."""
        from . import fewshot_ds as fd
        a = _host(qry_photometric_chain)
        if a.dtype.kind not in 'iuf' or a.ndim != 3 or a.shape[0] != rs['B'] or \
                not 1 <= a.shape[1] <= fd.PHOTO_CHAIN_MAX or a.shape[2] != len(fd.PHOTO_PARAMS):
            raise ValueError(f'qry_photometric_chain must be [B,P,{len(fd.PHOTO_PARAMS)}] numbers {fd.PHOTO_PARAMS} with P '
                             f'in 1..{fd.PHOTO_CHAIN_MAX} for {rs["B"]} images, got {a.dtype} {list(a.shape)}')
        recs = np.stack([fd.photometric_chain_records(c, hw, rs['hw']) for c, hw in zip(a, rs['sizes'])])
        if qry_augment is not None:
            for i, (g, hw) in enumerate(zip(_host(qry_augment), rs['sizes'])):
                if not fd.augment_is_neutral(fd.check_augment_params(g)) and not aug_recs[i, 2:6].any():
                    recs[i] = fd.photometric_chain_records(None, hw, rs['hw'])
        return FGN._chain_launch(recs)

    @staticmethod
    def _refuse_augment(**given) -> None:
        """The test path takes none of the augmentation arguments (by keyword, refused in the order given)."""
        for name, v in given.items():
            if v is not None:
                raise ValueError(f'{name} is for forward_train: the test is without augmentation')

    @staticmethod
    def _support_plans(spp_augment, spp_photometric, sp: dict, spp_photometric_chain=None) -> dict:
        """The contract of ``spp_augment`` / ``spp_photometric`` (host only, nothing is queued): [B,N*K,8] / [B,N*K,3]
        finite rows ([N*K,.] for a single support set) inside the sets and bounds of the queries' rows, at S -> S.  ``sp``:
        the dict of ``_source_supports``, whose boxes the plan starts from.  -> ``sp`` with ``boxes`` replaced by
        ``fewshot_ds.support_augment_plan``'s and, unless every instance is neutral after the per-instance fallback,
        ``aug`` int32 [n,16] and ``photo`` int32 [n,64] (None where every photometric record is neutral).
        ``spp_photometric_chain`` (in place of ``spp_photometric``): [B,N*K,P,3] ([N*K,P,3] for a single set), a chain per
        instance through ``fewshot_ds.support_augment_chain_plan``; ``photo`` is then ``_chain_launch`` of its records."""
        from . import fewshot_ds as fd
        B, n, S = sp['B'], sp['n'], sp['S']
        rows = {}
        chains = None
        if spp_photometric_chain is not None:
            chains = _host(spp_photometric_chain)
            width = len(fd.PHOTO_PARAMS)
            lead = tuple(chains.shape[:-2])
            if chains.dtype.kind not in 'iuf' or chains.ndim < 3 or chains.shape[-1] != width or \
                    not 1 <= chains.shape[-2] <= fd.PHOTO_CHAIN_MAX or \
                    not (lead == (B, n // B) or (B == 1 and lead == (n,))):
                raise ValueError(f'spp_photometric_chain must be [B,N*K,P,{width}] numbers {fd.PHOTO_PARAMS} with P in 1..'
                                 f'{fd.PHOTO_CHAIN_MAX} for {B} support set(s) of {n // B} instances ([N*K,P,{width}] for '
                                 f'a single set), got {chains.dtype} {list(chains.shape)}')
            chains = chains.reshape(n, chains.shape[-2], width)
        for name, v, width, fields in (('spp_augment', spp_augment, len(fd.AUG_PARAMS), fd.AUG_PARAMS),
                                       ('spp_photometric', spp_photometric, len(fd.PHOTO_PARAMS), fd.PHOTO_PARAMS)):
            if v is None:
                rows[name] = None
                continue
            rows[name] = _number_rows(
                v, ((B, n // B, width),) + (((n, width),) if B == 1 else ()),
                f'{name} must be [B,N*K,{width}] numbers {fields} for {B} support set(s) of {n // B} instances '
                f'([N*K,{width}] for a single set)').reshape(n, width)
        try:
            if chains is not None:
                recs, precs, boxes, _ = fd.support_augment_chain_plan(rows['spp_augment'], chains,
                                                                      sp['boxes'].numpy().reshape(n, 4), S)
            else:
                recs, precs, boxes, _ = fd.support_augment_plan(rows['spp_augment'], rows['spp_photometric'],
                                                                sp['boxes'].numpy().reshape(n, 4), S)
        except ValueError as e:             # (the rows' sets and bounds are the queries': name the supports' arguments)
            raise ValueError(str(e).replace('qry_augment', 'spp_augment').replace('qry_photometric', 'spp_photometric')
                             ) from None
        sp = dict(sp, boxes=torch.from_numpy(boxes.reshape(B, n // B, 4)))
        if chains is not None:
            photo = FGN._chain_launch(precs)
            if recs[:, 2:6].any() or photo is not None:
                sp.update(aug=torch.from_numpy(recs), photo=photo)
        elif recs[:, 2:6].any() or precs[:, 2].any():
            sp.update(aug=torch.from_numpy(recs), photo=torch.from_numpy(precs) if precs[:, 2].any() else None)
        return sp

    def _train_front(self, qry_img, qry_bboxes, qry_cat_ids, qry_isegmaps, qry_bboxes_ignore=None, proposals=None,
                     spp_imgs=None, spp_bboxes=None, spp_isegmaps=None, img_shape=None, qry_resize_to=None,
                     spp_crop_to=None, spp_fill_ratio: float = 0.8, crop_square: bool = True, qry_augment=None,
                     qry_photometric=None, spp_augment=None, spp_photometric=None, qry_photometric_chain=None,
                     spp_photometric_chain=None, **kwargs) -> dict:
        """The front of a training batch, shared by ``forward_train`` and ``train.Trainer``: the contracts of
        ``qry_resize_to``, ``spp_crop_to``, ``qry_augment``, ``qry_photometric``, ``spp_augment``, ``spp_photometric``,
        ``qry_photometric_chain`` and ``spp_photometric_chain`` (every error before anything is queued), then the uploads
        and the kernels behind them.  -> the keyword arguments of ``train.forward_train``."""
        for single, chain, s, c in (('qry_photometric', 'qry_photometric_chain', qry_photometric, qry_photometric_chain),
                                    ('spp_photometric', 'spp_photometric_chain', spp_photometric, spp_photometric_chain)):
            if s is not None and c is not None:
                raise ValueError(f'{single} and {chain} are two forms of one argument: give one operator per image '
                                 f'({single}) or a chain of them ({chain}), not both')
        for name, v in (('spp_augment', spp_augment), ('spp_photometric', spp_photometric),
                        ('spp_photometric_chain', spp_photometric_chain)):
            if v is not None and spp_crop_to is None:
                raise ValueError(f'{name} needs spp_crop_to: the supports are augmented on the device behind their cut '
                                 f'from the source images')
        if qry_augment is not None and qry_resize_to is None:
            raise ValueError('qry_augment needs qry_resize_to: the query is augmented together with its resize from the '
                             'source size')
        if qry_photometric is not None and qry_resize_to is None:
            raise ValueError('qry_photometric needs qry_resize_to: the photometric operators run on the source pixels, '
                             'ahead of their resize')
        if qry_photometric_chain is not None and qry_resize_to is None:
            raise ValueError('qry_photometric_chain needs qry_resize_to: the photometric operators run on the source '
                             'pixels, ahead of their resize')
        qry_isegmaps = self._gt_front(qry_isegmaps, qry_img, img_shape, qry_resize_to)
        sp = None
        if spp_crop_to is None:
            _dense_supports_only(spp_isegmaps)
        else:                                             # (every contract error before anything is queued)
            sp = self._source_supports(spp_imgs, spp_bboxes, spp_isegmaps, spp_crop_to, spp_fill_ratio, crop_square)
            if spp_augment is not None or spp_photometric is not None or spp_photometric_chain is not None:
                sp = self._support_plans(spp_augment, spp_photometric, sp, spp_photometric_chain)
        rs = recs = precs = None
        if qry_resize_to is not None:
            rs = self._source_query(qry_img, qry_resize_to, img_shape, qry_isegmaps)
            if qry_augment is not None:
                recs, boxes = self._augment_plans(qry_augment, qry_bboxes, rs)
            if qry_photometric is not None:
                precs = self._photometric_records(qry_photometric, rs, qry_augment,
                                                  None if recs is None else recs.numpy())
            if qry_photometric_chain is not None:
                precs = self._photometric_chain_records(qry_photometric_chain, rs, qry_augment,
                                                        None if recs is None else recs.numpy())
        if rs is not None or sp is not None:
            dev = self._gpu('forward_train')
        if rs is None and _has_color(qry_isegmaps):
            # uint8 pixels at the network size: up on this stream, the masks made right behind the copy
            dev = self._gpu('forward_train')
            qry_img = qry_img.to(dev, non_blocking=True).contiguous()
            qry_isegmaps = self._color_on_device(qry_isegmaps, qry_img.view(qry_img.shape[0], -1))
        if rs is not None:
            qry_img = _InputForm(source=rs).query(self._upload_source(rs, dev))
            # box + colour entries: from the bytes AS UPLOADED, ahead of the photometric pass (which writes a new tensor;
            # the reference derives its masks before it augments, mnistiseg_ds.py:124-132)
            qry_isegmaps = self._color_on_device(qry_isegmaps, qry_img.src)
            if precs is not None:                          # (all rows neutral after the fallback: no launch)
                run = ops.photometric_u8 if precs.dim() == 2 else ops.photometric_chain_u8      # ([B,64] or [B,P,64])
                qry_img = qry_img._replace(src=run(qry_img.src, precs.to(dev, non_blocking=True)))
            if recs is None:
                qry_bboxes = self._scaled_boxes(qry_bboxes, rs['sizes'], rs['hw'])
                qry_isegmaps = [self._resized_masks(g, rs['hw'], dev) for g in qry_isegmaps]
            else:
                qry_img = qry_img._replace(rec=recs.to(dev, non_blocking=True))
                qry_bboxes = boxes
                plain = [not bool(r[2:6].any()) for r in recs.numpy()]          # neutral, or fallen back
                qry_isegmaps = [self._resized_masks(g, rs['hw'], dev) if p else
                                self._augmented_masks(g, qry_img.rec[i], rs['hw'], dev)
                                for i, (g, p) in enumerate(zip(qry_isegmaps, plain))]
            img_shape = rs['img_shape']
        if sp is not None:
            (spp_imgs, spp_bboxes), spp_isegmaps = self._supports_on_device(sp, dev), None
        return dict(qry_img=qry_img, qry_bboxes=qry_bboxes, qry_cat_ids=qry_cat_ids, qry_isegmaps=qry_isegmaps,
                    qry_bboxes_ignore=qry_bboxes_ignore, proposals=proposals, spp_imgs=spp_imgs, spp_bboxes=spp_bboxes,
                    spp_isegmaps=spp_isegmaps, img_shape=img_shape, **kwargs)

    @staticmethod
    def _gpu(entry: str) -> torch.device:
        """The current device of an entry point that is about to queue work (every contract error comes before)."""
        if not torch.cuda.is_available():
            raise ops._lib.FgnHipError(f'FGN.{entry} needs a GPU: the HIP path has no CPU fallback')
        return torch.device('cuda', torch.cuda.current_device())

    @staticmethod
    def _scaled_boxes(qry_bboxes, sizes, hw):
        """The boxes of source-size queries at the network size, exactly as ``fewshot_ds.resize_query`` scales them
        (base_fst.py:877-878; the caller's arrays are never written; untouched at equal size)."""
        if qry_bboxes is None:
            return None
        from .fewshot_ds import scale_boxes_yxyx
        out = []
        for b, (h, w) in zip(qry_bboxes, sizes):
            if (h, w) == tuple(hw) or b is None:
                out.append(b)
            else:
                nb = scale_boxes_yxyx(_host(b), h, w, *hw)
                out.append(torch.from_numpy(nb) if isinstance(b, torch.Tensor) else nb)
        return out

    def _source_supports(self, spp_imgs, spp_bboxes, spp_isegmaps, spp_crop_to, spp_fill_ratio: float = 0.8,
                         crop_square: bool = True, graphed: bool = False) -> dict:
        """The contract of ``spp_crop_to`` (host only, nothing is queued): S is an int, a table is set, ``spp_imgs`` is
        a list of N*K uint8 images [h_i,w_i,3] (or B such lists), ``spp_isegmaps`` has the same nesting with every mask
        at its image's size, ``spp_bboxes`` holds one YXYX box per instance, inside its image and not empty
        (``fewshot_ds.support_geometry``), and every window fits the slot.  -> B, n = B*N*K, S, the records int32 [n,16],
        the boxes in the S x S supports float32 (``support_from_instance``'s, computed here on the host) [B,N*K,4], the
        image and mask windows as flat byte tensors, the largest of each and the slot sizes in bytes per instance.  A mask
        may be ONE mask in a compact form (``maskforms.checked_one``) in its image's frame: the geometry is the same, its
        entry of ``mflats`` is empty - no mask byte is uploaded -, ``mrle`` / ``mpoly`` list (row, carrier, window) and
        ``mcol`` lists (row, the colour item moved into the window's frame, which must hold its whole box) for
        ``_upload_supports``, and ``window_bytes`` counts what crosses the bus instead (``Form.nbytes``)."""
        from . import fewshot_ds as fd
        if isinstance(spp_crop_to, bool) or not isinstance(spp_crop_to, (int, np.integer)) or \
                not 1 <= int(spp_crop_to) <= ops.RESIZE_MAX_DIM:
            raise ValueError(f'spp_crop_to must be an int within 1..{ops.RESIZE_MAX_DIM} (the support size S), got '
                             f'{spp_crop_to!r}')
        S = int(spp_crop_to)
        if self.input_lut is None:
            raise ValueError('spp_crop_to needs the normalisation table: call set_input_norm first')
        NK = self.n_ways * self.k_shots
        nested = lambda v: isinstance(v, (list, tuple)) and len(v) > 0 and isinstance(v[0], (list, tuple)) and \
            not maskforms.is_pair(v[0])                    # (a ``[size, counts]`` pair is one mask, not a support set)
        if not isinstance(spp_imgs, (list, tuple)) or not isinstance(spp_isegmaps, (list, tuple)):
            raise ValueError('spp_imgs / spp_isegmaps: with spp_crop_to, lists of N*K source images [h,w,3] and masks '
                             '[h,w] (or B such lists)')
        if nested(spp_imgs) != nested(spp_isegmaps):
            raise ValueError('spp_imgs and spp_isegmaps must be nested alike')
        groups = list(zip(spp_imgs, spp_isegmaps)) if nested(spp_imgs) else [(spp_imgs, spp_isegmaps)]
        B = len(groups)
        if len(spp_isegmaps) != len(spp_imgs) or any(len(g[0]) != NK or len(g[1]) != NK for g in groups):
            raise ValueError(f'spp_imgs / spp_isegmaps: every support set holds N*K = {NK} images and as many masks')
        bb = _host(spp_bboxes)
        if bb.size != B * NK * 4 or bb.shape[-1] != 4:
            raise ValueError(f'spp_bboxes: with spp_crop_to, [..,{NK},4] YXYX in the source frame for {B} support '
                             f'set(s), got {list(bb.shape)}')
        bb = bb.reshape(B * NK, 4)
        recs, boxes, wins, compact = [], [], [], {f: [] for f in maskforms.FORMS}
        for i, (im, mk) in enumerate((im, mk) for g in groups for im, mk in zip(*g)):
            im = _host(im)
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
                raise ValueError(f'spp_imgs: with spp_crop_to every image is channels-last uint8 pixels [h,w,3], got '
                                 f'{im.dtype} {list(im.shape)}')
            form = maskforms.form_of_one(mk)
            if form is not None:        # ONE mask in a compact form, in its image's frame: no mask byte is uploaded
                one = maskforms.checked_one(mk, im.shape[:2], f'spp_isegmaps[{i}]')
                mk = np.zeros((0, 0), np.uint8)
            else:
                mk = _host(mk)
                if mk.shape != im.shape[:2]:
                    raise ValueError(f'spp_isegmaps: with spp_crop_to every mask is at its image\'s size '
                                     f'{list(im.shape[:2])}, got {list(mk.shape)}')
            rec, box = fd.support_geometry(im.shape[0], im.shape[1], bb[i], S, spp_fill_ratio, crop_square)
            recs.append(rec); boxes.append(box); wins.append(fd.support_window(im, mk, rec))
            if form is not None:        # its window is decoded, rasterised or made into row i (_upload_supports)
                g = dict(zip(fd.SPP_REC_FIELDS, (int(v) for v in rec)))
                win = (g['wy'], g['wx'], g['wh'], g['ww'])
                # (colour: ``support_geometry``'s crop reads the rows and columns of the instance's box unreflected, so
                # the window holds the whole box; the item travels in the window's frame, beside the image window)
                compact[form].append((i, one.in_window(*win, f'spp_isegmaps[{i}]', f'the crop of spp_bboxes[{i}]'))
                                     if form is maskforms.COLOR else (i, one, win))
        need = max(w[0].size for w in wins)
        mneed = need // 3                                  # (wh * ww of the largest window, dense or not)
        capacity, mcapacity = need, mneed
        if graphed:
            capacity = int(self.support_source_capacity)
            mcapacity = capacity // 3
            if need > capacity or mneed > mcapacity:
                raise ValueError(f'a support window of {need} bytes exceeds FGN.support_source_capacity = {capacity}: '
                                 f'raise the attribute (the static window slot of the captured graph)')
        return dict(B=B, n=B * NK, S=S, rec=torch.from_numpy(np.stack(recs)),
                    boxes=torch.from_numpy(np.stack(boxes).reshape(B, NK, 4)),
                    flats=[torch.from_numpy(w.reshape(-1)) for w, _ in wins],
                    mflats=[torch.from_numpy(m.reshape(-1)) for _, m in wins], need=need, mneed=mneed,
                    capacity=capacity, mcapacity=mcapacity, mrle=compact[maskforms.RLE], mcol=compact[maskforms.COLOR],
                    mpoly=compact[maskforms.POLY],
                    window_bytes=int(sum(w.size + m.size for w, m in wins) +
                                     sum(f.nbytes(item[1]) for f, items in compact.items() for item in items)))

    @staticmethod
    def _slot_rows(flats: list, width: int, capacity: int, dev, slot: Optional[torch.Tensor]) -> torch.Tensor:
        """Flat byte tensors into the fronts of the rows of ``slot`` (a static slot of a captured graph) when that is
        given at [len(flats), capacity], else of a fresh buffer ``width`` wide, on the current stream."""
        if slot is None or tuple(slot.shape) != (len(flats), capacity):
            slot = torch.empty((len(flats), width), dtype=torch.uint8, device=dev)
        for i, flat in enumerate(flats):
            slot[i, :flat.numel()].copy_(flat, non_blocking=True)
        return slot

    def _upload_supports(self, sp: dict, dev, into: Optional[dict] = None) -> dict:
        """The windows of ``_source_supports`` on the device, on the current stream: wh_i * ww_i * 3 image bytes and
        wh_i * ww_i mask bytes of instance i into row i of ``into['spp_src']`` / ``into['spp_msk']`` (the static slots of
        a captured graph) when those are given, else of fresh buffers as wide as the largest window of the batch - only
        the window bytes cross the bus, and what lies behind a window in its row is never read.  The window of an
        instance whose mask came as RLE (``sp['mrle']``) is decoded on the device into its row, right where the copy would
        have stood (``ops.rle_decode_rows``: one launch for all of them).  -> the two by name."""
        into = into or {}
        msk = self._slot_rows(sp['mflats'], sp['mneed'], sp['mcapacity'], dev, into.get('spp_msk'))
        # an instance whose mask came as RLE uploaded no mask byte: its window is decoded straight into its row
        ops.rle_decode_rows(msk, sp.get('mrle') or [])
        # ... and one that came as polygons is rasterised into its row (one upload, two launches for all)
        ops.poly_mask_rows(msk, sp.get('mpoly') or [])
        src = self._slot_rows(sp['flats'], sp['need'], sp['capacity'], dev, into.get('spp_src'))
        if sp.get('mcol'):
            # ... and one that came as box + colour has its mask made from its image window, on this stream BEHIND the
            # copy of that window and ahead of the cut that reads both
            ops.color_mask_rows(src, msk, sp['mcol'])
        return {'spp_src': src, 'spp_msk': msk}

    def _supports_on_device(self, sp: dict, dev) -> tuple:
        """``_source_supports`` uploaded on the current stream, in the form ``_support_front`` takes:
        (``_SupportWindows``, the boxes) - with the records of ``_support_plans`` where an instance is augmented."""
        s = _InputForm(spp_source=sp).supports(dict(self._upload_supports(sp, dev), spp_rec=sp['rec']))
        return s._replace(aug=sp.get('aug'), photo=sp.get('photo')).to(dev), sp['boxes']

    # --- stages ---------------------------------------------------------------------------
    def extract_feat(self, img: Union[torch.Tensor, '_QueryPixels']) -> torch.Tensor:
        """ResNet-50 stages 1-3 (fgn.py:67-77): NCHW fp32 (or uint8 pixels, ``set_input_norm``) in, NHWC [B,h,w,1024]
        out."""
        P = self._P
        bb = self.cfg['backbone']
        x = self._stem_input(img)
        for conv, gn in P['stem']:
            x = ops.conv2d(x, conv)
            if gn is not None:
                x = ops.group_norm(x, gn[0], gn[1], bb.get('gn_groups', 32), bb['bn_eps'], relu=True, inplace=True)
        x = ops.maxpool3x3s2(x)
        for stage in P['stages']:
            for blk in stage:
                x = blk(x)
        return x

    def extract_feat_pair(self, qry: Union[torch.Tensor, '_QueryPixels'], spp: torch.Tensor, phase_counter=None):
        """Both backbone passes of an episode (fgn.py:212-215) through SHARED launches wherever a layer does not look at
        the spatial structure (``use_merged_backbone``; frozen-BN bottleneck backbones only)."""
        P = self._P
        outs = [self._stem_input(img) for img in (qry, spp)]
        for conv, _ in P['stem']:
            y = [torch.empty((o.shape[0], (o.shape[1] + 2 * conv.pad - conv.kh) // conv.stride + 1,
                              (o.shape[2] + 2 * conv.pad - conv.kw) // conv.stride + 1, conv.cout), device=o.device,
                             dtype=torch.float32) for o in outs]
            _conv_pair(outs[0], outs[1], conv, y[0], y[1])
            outs = y
        hw = lambda t: ((t.shape[1] - 1) // 2 + 1, (t.shape[2] - 1) // 2 + 1)
        x = _Pair((outs[0].shape[0],) + hw(outs[0]), (outs[1].shape[0],) + hw(outs[1]), outs[0].shape[3], outs[0].device)
        ops.maxpool3x3s2(outs[0], out=x.q)
        ops.maxpool3x3s2(outs[1], out=x.s)
        self._phase_mark('layer1', phase_counter)    # (stem + max-pool done)
        for si, stage in enumerate(P['stages']):
            for blk in stage:
                x = _bottleneck_pair(blk, x)
            self._phase_mark('layer%d' % (si + 2), phase_counter)     # 'layer2' = layer1 done, ..., the last stage's mark equals 'rpn'
        return x.q, x.s

    def _shared_head(self, x, n_img_dev=None, y1=None):
        for bi, blk in enumerate(self._P['shared']):
            x = blk(x, n_img_dev, y1=y1 if bi == 0 else None)
        return x

    def _roi_feats(self, fmap, g_map, rois, n_dev):
        """RoIAlign of the C4 map + the shared_head (fgn_roi_head.py:331-336 / 366-369).  RoIAlign is linear per
        channel, so the first 1x1 conv of the shared_head is taken on the feature map (``g_map``, once per episode,
        50x84 pixels instead of 49 per RoI) and only its BN shift + ReLU follow the pooling."""
        P, rh = self._P, self.cfg['roi_head']
        PS, inv = rh['roi_out_size'], 1.0 / rh['featmap_stride']
        if g_map is not None:       # both maps at the same sampling points: one launch
            x, y1 = ops.roi_align2(fmap, g_map, rois, PS, inv, rh['roi_sampling_ratio'], True, n_dev,
                                   post_shift2=P['sh0_shift'], relu2=True)
        else:
            x, y1 = ops.roi_align(fmap, rois, PS, inv, rh['roi_sampling_ratio'], True, n_dev), None
        return x, self._shared_head(x, n_dev, y1=y1)

    def _mask_head(self, mf, vmask, n_dev=None, prob_out=None):
        """``_mask_forward`` after the shared_head (fgn_roi_head.py:379-380): support-vector guidance, FCNMaskHead
        (4 x conv3x3+ReLU, ConvTranspose 2x2/2 + ReLU as one 1x1 conv with 4*C' outputs, 1x1 logits), sigmoid.
        mf [D,7,7,C], vmask [D,C] -> logits, probabilities [D,14,14]."""
        P = self._P
        m = mf
        for li, (layer, wg) in enumerate(zip(P['mask_convs'], P['mask_convs_wg'])):
            scale = vmask if li == 0 else None         # support-vector guidance (fgn_roi_head.py:379) fused into conv 0
            if wg is not None and ops.winograd_pays(m.shape[0], m.shape[1], m.shape[2], wg.cin, wg.cout, wg.m):
                m = ops.conv3x3_winograd(m, wg, in_scale=scale, n_img_dev=n_dev)
            else:
                m = ops.conv2d(m, layer, in_scale=scale, n_img_dev=n_dev)
        up = ops.conv2d(m, P['upsample'], n_img_dev=n_dev)                         # [D,7,7,4*C']
        return ops.mask_logits(up, P['logit_w'], P['logit_b'], self.cfg['roi_head']['roi_out_size'], n_dev,
                               prob_out=prob_out)

    def forward(self, return_loss=True, **kwargs):
        if return_loss:
            return self.forward_train(**kwargs)
        return self.simple_test(**kwargs)

    @torch.no_grad()
    def forward_train(self, qry_img, qry_bboxes, qry_cat_ids, qry_isegmaps, qry_bboxes_ignore=None, proposals=None,
                      spp_imgs=None, spp_bboxes=None, spp_isegmaps=None, img_shape=None, qry_resize_to=None,
                      spp_crop_to=None, spp_fill_ratio: float = 0.8, crop_square: bool = True, qry_augment=None,
                      qry_photometric=None, spp_augment=None, spp_photometric=None, qry_photometric_chain=None,
                      spp_photometric_chain=None, **kwargs) -> Dict:
        """The loss dict of one training step (fgn.py:125-185) as forward values - see ``fgn_amd.train``.  Keys and
        container types are the reference's: ``loss_rpn_cls`` / ``loss_rpn_bbox`` (lists of one tensor),
        ``loss_cls``, ``ACC-Unbalanced``, ``ACC-Balanced``, ``loss_bbox``, ``loss_mask``.  ``qry_resize_to``: source-size
        query images, masks and boxes, as for ``simple_test``; ``spp_crop_to``: supports cut from their source images on
        the device, as for ``simple_test``.  ``qry_augment`` (needs ``qry_resize_to``): [B,8] rows of
        ``fewshot_ds.AUG_PARAMS`` - flip, rotation, scale, shear, translation, border, channel order - applied to image
        and masks on the device together with the resize (``fewshot_ds.augment_query`` bit for bit; ``get_query`` with
        ``augment_qry``, base_fst.py:889-891), to the boxes on the host; an image whose boxes leave it is
        used un-augmented, as in the reference.  ``qry_photometric`` (needs ``qry_resize_to``, with or without
        ``qry_augment``): [B,3] rows of ``fewshot_ds.PHOTO_PARAMS`` - one of Gaussian noise, impulse noise, Gaussian blur,
        hue, saturation, brightness per image, applied to the source pixels on the device ahead of the resize
        (``fewshot_ds.photometric_image_u8`` bit for bit); an image whose boxes leave it under
        ``qry_augment`` is used without either.  ``spp_augment`` / ``spp_photometric`` (need ``spp_crop_to``; either
        without the other): [B,N*K,8] / [B,N*K,3] rows of the same two formats, one pair per support INSTANCE, applied on
        the device to the S x S crop behind its cut - after resize and pad, the reference's own order
        (``fewshot_ds.augment_support`` bit for bit; ``get_support`` with ``augment_spp``, base_fst.py:1151-1153;
        DESIGN 4.4.7) - and to ``spp_bboxes`` on the host; an instance whose box leaves its crop is used un-augmented,
        that instance alone.  At most three launches make the supports, whatever N*K.  ``qry_photometric_chain`` [B,P,3]
        / ``spp_photometric_chain`` [B,N*K,P,3] (P in 1..3; each in place of its single-operator sibling, never beside
        it): a chain of rows per image or instance, applied in order - point operators, then at most one blur, COCO's
        ``augs_seq`` (coco_ds.py:45-59) - in the same place and in one launch that reads and writes every image once
        (``fewshot_ds.photometric_chain_u8`` bit for bit).  A batch whose chains hold at most one active
        operator each makes exactly the single-operator launch, an all-neutral one none."""
        from . import train
        return train.forward_train(self, **self._train_front(
            qry_img, qry_bboxes, qry_cat_ids, qry_isegmaps, qry_bboxes_ignore=qry_bboxes_ignore, proposals=proposals,
            spp_imgs=spp_imgs, spp_bboxes=spp_bboxes, spp_isegmaps=spp_isegmaps, img_shape=img_shape,
            qry_resize_to=qry_resize_to, spp_crop_to=spp_crop_to, spp_fill_ratio=spp_fill_ratio, crop_square=crop_square,
            qry_augment=qry_augment, qry_photometric=qry_photometric, spp_augment=spp_augment,
            spp_photometric=spp_photometric, qry_photometric_chain=qry_photometric_chain,
            spp_photometric_chain=spp_photometric_chain, **kwargs))

    @torch.no_grad()
    def simple_test(self, qry_img, qry_bboxes=None, qry_cat_ids=None, qry_isegmaps=None, qry_bboxes_ignore=None,
                    spp_imgs=None, spp_bboxes=None, spp_isegmaps=None, qry_child_idx=None, img_shape=None,
                    rescale=False, cats_ids_to_sample_real=None, spp_insts_ids=None, idx=None,
                    support_code=None, qry_resize_to=None, results_at_source: bool = False, spp_crop_to=None,
                    spp_fill_ratio: float = 0.8, crop_square: bool = True, qry_augment=None, qry_photometric=None,
                    spp_augment=None, spp_photometric=None, qry_photometric_chain=None, spp_photometric_chain=None,
                    **kwargs) -> List[Dict]:
        """Test without augmentation (fgn.py:187-303; ``qry_augment``, ``qry_photometric``, ``spp_augment``,
        ``spp_photometric`` and the two ``*_photometric_chain`` are refused).  ``support_code`` (optional, from
        ``encode_supports``) replaces the three ``spp_*`` inputs.  ``qry_resize_to`` = (H, W) (or a [B,2] tensor of
        equal rows): ``qry_img`` holds decoded images at their SOURCE size - a uint8 tensor [B,h,w,3] or a list of B
        uint8 tensors [h_i,w_i,3] - and ``qry_isegmaps`` / ``qry_bboxes`` are at source size too; image and masks are
        resized to the network size on the device (``fewshot_ds.resize_query`` bit for bit, base_fst.py:876-887), the
        boxes on the host; needs ``set_input_norm``.  ``results_at_source`` (needs ``qry_resize_to``; ``rescale`` stays
        accepted and ignored): every quantity of a result dict is in the frame of its SOURCE image -
        ``dt_bboxes`` divided by the image's scale (``fewshot_ds.boxes_to_source``), ``dt_isegmaps_rle`` pasted at
        ``[h_b, w_b]`` from those boxes, the ground truth encoded and counted as given (no mask resize), ``qry_bboxes``
        as given, ``qry_img_shape`` = ``[h_b, w_b, 3]``; the detections, their scores and their order are those of the
        call without it.  ``spp_crop_to`` = S (an int; with ``spp_fill_ratio`` and ``crop_square`` of the dataset): the
        supports come as their SOURCE images - ``spp_imgs`` a list of N*K uint8 tensors [h_i,w_i,3] of any sizes (or B
        such lists), ``spp_isegmaps`` the instances' masks [h_i,w_i] nested alike, ``spp_bboxes`` [..,N*K,4] YXYX in the
        source frame - and crop, bicubic resize and centre pad of ``BaseFewShotISEG.get_support`` (base_fst.py:1043-1167)
        run on the device in one launch (``fewshot_ds.support_from_source`` bit for bit); only the window
        of each image that its crop reads is uploaded; needs ``set_input_norm``.  Masks as COCO RLE: every
        entry of ``qry_isegmaps`` may be a list of RLE items (``rle.as_masks``: pycocotools dicts or ``[size, counts]``
        pairs; at the image's source size with ``qry_resize_to``, else at the network size; dense and RLE entries may be
        mixed in a batch), and with ``spp_crop_to`` every instance of ``spp_isegmaps`` may be one RLE item at its source
        image's size; they are checked on the host, only their runs are uploaded and the device decodes them into the
        bytes of the dense form - every result is that of the dense call.  Masks as box + colour, the
        form the character datasets store: an entry of ``qry_isegmaps`` may be a ``colormask.ColorMasks`` or a dict
        ``{'bboxes': [n,4] YXYX, 'colors': [n,3] RGB[, 'shift']}`` in the frame of the image as handed over (source size
        with ``qry_resize_to``, else the network size), mixed freely with the other two forms; it needs the image as
        uint8 pixels (``set_input_norm``; a float image is refused), and with ``spp_crop_to`` every instance of
        ``spp_isegmaps`` may be one such item in its source image's frame.  The device makes the masks from the image
        bytes it was sent anyway, on the stream that carried them and behind their copy; 16 ints per mask are uploaded.
        Masks as COCO polygons: an entry of ``qry_isegmaps`` may be a ``polygon.PolyMasks`` or a dict
        ``{'polygons': [instance, ...][, 'size': [h, w]]}``, every instance a list of parts ``[x0, y0, x1, y1, ...]`` as
        COCO's ``segmentation`` holds them, in the same frame, mixed freely with the other forms - never a bare nested
        list - and with ``spp_crop_to`` every instance of ``spp_isegmaps`` may be ``{'polygons': parts}``; the vertices
        are checked on the host, uploaded as records and rasterised on the device into the bytes ``polygon.dense`` gives."""
        self._refuse_augment(qry_augment=qry_augment, qry_photometric=qry_photometric, spp_augment=spp_augment,
                             spp_photometric=spp_photometric, qry_photometric_chain=qry_photometric_chain,
                             spp_photometric_chain=spp_photometric_chain)
        if results_at_source and qry_resize_to is None:
            raise ValueError('results_at_source needs qry_resize_to: results at source size exist for source-size queries')
        qry_isegmaps = self._gt_front(qry_isegmaps, qry_img, img_shape, qry_resize_to)
        sp = None
        if spp_crop_to is not None and support_code is None:
            sp = self._source_supports(spp_imgs, spp_bboxes, spp_isegmaps, spp_crop_to, spp_fill_ratio, crop_square,
                                       self._graphed())
        if qry_resize_to is None:
            dets = self.detect_device(qry_img, spp_imgs, spp_bboxes, spp_isegmaps, img_shape, support_code,
                                      qry_isegmaps=qry_isegmaps, spp_crop_to=sp, qry_bboxes=qry_bboxes,
                                      qry_cat_ids=qry_cat_ids)
            batch = qry_img.shape[0]
        else:
            rs = self._source_query(qry_img, qry_resize_to, img_shape, qry_isegmaps, self._graphed())
            if not results_at_source:       # (host only: the boxes of the result dicts, which the device matches against)
                qry_bboxes = self._scaled_boxes(qry_bboxes, rs['sizes'], rs['hw'])
            dets = self.detect_device(qry_img, spp_imgs, spp_bboxes, spp_isegmaps, img_shape, support_code,
                                      qry_isegmaps=qry_isegmaps, qry_resize_to=rs, results_at_source=results_at_source,
                                      spp_crop_to=sp, qry_bboxes=qry_bboxes, qry_cat_ids=qry_cat_ids)
            batch, img_shape = rs['B'], rs['img_shape']
        return self.pack_results(dets, batch, qry_bboxes=qry_bboxes, qry_cat_ids=qry_cat_ids,
                                 qry_isegmaps=qry_isegmaps, img_shape=img_shape, qry_child_idx=qry_child_idx,
                                 cats_ids_to_sample_real=cats_ids_to_sample_real, spp_insts_ids=spp_insts_ids,
                                 idx=idx, qry_resize_to=None if qry_resize_to is None else rs['hw'],
                                 results_at_source=results_at_source)

    # --- support branch (fgn.py:212-215 backbone pass; fgn_ag_rpn_head.py:38-41; fgn_roi_head.py:419-449) ---
    def _support_front(self, spp_imgs, spp_bboxes, spp_isegmaps, B, dev, stream, defer_backbone: bool = False) -> dict:
        """modify_input for the supports (fgn.py:79-108: H2D, YXYX -> XYXY on private copies), their
        backbone pass and the AG-RPN class vectors."""
        N, K = self.n_ways, self.k_shots
        windows = isinstance(spp_imgs, _SupportWindows)         # windows of the source images (``spp_crop_to``)
        if not windows:
            self._image_dims(spp_imgs, 'spp_imgs', lead=(1, 2))
        b = spp_bboxes.to(dev, torch.float32, non_blocking=True).reshape(B * N * K, 4)
        spp_xyxy = torch.stack((b[:, 1], b[:, 0], b[:, 3], b[:, 2]), 1)      # no host-built index tensor: graph-capturable
        if windows:
            s = spp_imgs.to(dev)
            if s.src.shape[0] != B * N * K:
                raise ValueError(f'{s.src.shape[0]} support instances for a batch of {B} x {N} x {K}')
            y, spp_masks = s.stem_input(self._lut_on(dev))
            spp = _StemReady(y)
        else:
            spp = spp_imgs.to(dev, non_blocking=True).reshape(B * N * K, *spp_imgs.shape[-3:])    # (dtype: _stem_input)
            m = spp_isegmaps.to(dev, non_blocking=True).reshape(B * N * K, *spp_isegmaps.shape[-2:])
            spp_masks = (m.view(torch.uint8) if m.dtype == torch.bool else m.to(torch.uint8)).contiguous()
        sc = dict(B=B, device=dev, spp_xyxy=spp_xyxy, spp_masks=spp_masks, spp=spp)
        if not defer_backbone:
            self._support_vectors(sc, self.extract_feat(sc.pop('spp')))         # [B*N*K,s,s,C]
        return sc

    def _support_vectors(self, sc: dict, spp_fmaps) -> None:
        sc['spp_fmaps'] = spp_fmaps
        sc['vec'] = ops.support_class_vectors(spp_fmaps, None, sc['B'] * self.n_ways, self.k_shots)   # [B*N,C]

    def _support_back(self, sc: dict, B, dev, shared=None) -> None:
        """count_spp (fgn_roi_head.py:419-449) and the support half of the relation conv.  ``shared``: the shared-head
        callable (forward_train passes the train-mode BatchNorm variant)."""
        sfeat = self._support_pool(sc, B, dev)
        self._support_finish(sc, self._shared_head(sfeat) if shared is None else shared(sfeat), B)

    def _support_pool(self, sc: dict, B, dev, out=None) -> torch.Tensor:
        """The support RoIs (image index | XYXY), the masks pooled on them (``sc['masks7']``) and the support maps pooled
        on them (into ``out`` when given)."""
        rh = self.cfg['roi_head']
        bidx = torch.arange(B * self.n_ways * self.k_shots, device=dev, dtype=torch.float32)[:, None]
        spp_rois = torch.cat([bidx, sc['spp_xyxy']], 1).contiguous()
        sc['masks7'] = ops.roi_align_mask(sc['spp_masks'], spp_rois, rh['roi_out_size'], 1.0, -1, False)
        # `spp_bboxes /= 16` then roi_align(scale=1) == roi_align(scale=1/16): /16 is exact in fp32
        return ops.roi_align(sc['spp_fmaps'], spp_rois, rh['roi_out_size'], 1.0 / rh['featmap_stride'], -1, False,
                             out=out)

    def _support_rois(self, sc: dict, B, dev, x_out, y1_out) -> None:
        """First half of count_spp for the MERGED shared head: the support masks and maps are pooled (into the first rows
        of the RoI batch the box head will run, ``x_out``), and - the first 1x1 conv of the shared head being taken on
        the feature map for the query's RoIs - the same conv on the pooled support features fills their rows of
        ``y1_out``."""
        self._support_pool(sc, B, dev, out=x_out)
        if y1_out is not None:
            ops.conv2d(x_out, self._P['shared'][0].conv1, out=y1_out)

    def _support_finish(self, sc: dict, sfeat, B) -> None:
        """Second half of count_spp (fgn_roi_head.py:439-447) + the support half of the relation conv, on the support
        rows of the shared head's output."""
        P, N, K = self._P, self.n_ways, self.k_shots
        sc['cat_mean'] = ops.support_kmean(sfeat, B * N, K)                           # [B*N,7,7,C]
        sc['cat_mean_mp'] = ops.support_class_vectors(sfeat, sc['masks7'], B * N, K)  # [B*N,C]
        sc['S'] = ops.conv2d(sc['cat_mean'], P['rel_s'])                              # Ws*support + bias

    @torch.no_grad()
    def encode_supports(self, spp_imgs, spp_bboxes, spp_isegmaps, spp_crop_to=None, spp_fill_ratio: float = 0.8,
                        crop_square: bool = True, spp_augment=None, spp_photometric=None,
                        spp_photometric_chain=None) -> dict:
        """Support-feature caching across queries: everything the path derives
        from the support set alone - backbone pass, AG-RPN class vectors, count_spp, the support
        half of the relation conv - computed once on the current stream.  The returned code is
        passed as ``support_code=`` to ``simple_test`` / ``detect_device`` for every query that
        shares the support set (the reference recomputes it per query, fgn.py:212-215; results
        are identical).  ``spp_crop_to``: the supports come as their source images, as for ``simple_test``.
        ``spp_augment`` / ``spp_photometric`` / ``spp_photometric_chain`` are refused: the test path is without
        augmentation."""
        self._refuse_augment(spp_augment=spp_augment, spp_photometric=spp_photometric,
                             spp_photometric_chain=spp_photometric_chain)
        sp = None
        if spp_crop_to is None:
            _dense_supports_only(spp_isegmaps)
        else:
            sp = self._source_supports(spp_imgs, spp_bboxes, spp_isegmaps, spp_crop_to, spp_fill_ratio, crop_square)
        dev = self._gpu('encode_supports')
        if self._packed_device != dev:
            self._pack(dev)
        self._sync_trained_shared()
        if sp is not None:
            B, ((spp_imgs, spp_bboxes), spp_isegmaps) = sp['B'], (self._supports_on_device(sp, dev), None)
        else:
            B = spp_imgs.shape[0] if spp_imgs.dim() == 5 else 1
        sc = self._support_front(spp_imgs, spp_bboxes, spp_isegmaps, B, dev, torch.cuda.current_stream())
        self._support_back(sc, B, dev)
        return sc

    def _sync_trained_shared(self) -> None:
        """A ``fgn_amd.train.Trainer`` updates the head layers in place after every step; the inference form of the
        shared head (eval-mode BatchNorm folded from the CURRENT weights and running statistics) is rebuilt here, on
        the first inference call after a training step, so ``simple_test`` always sees the trainer's weights."""
        src = getattr(self, '_shared_dirty', None)
        if src is not None:
            for k, v in self._pack_shared(src).items():
                self._P[k] = v
            self._shared_dirty = None
            self._graphs = {}

    def _stream_for(self, role: str, main) -> 'torch.cuda.Stream':
        """One auxiliary HIP stream per (role, caller stream), or what ``transfer_mode`` prescribes for the 'upload' and
        'copy' roles (``transfer_stream``).

        HIP maps streams onto a small pool of hardware queues (GPU_MAX_HW_QUEUES, 4 by default; the k-th stream created
        takes queue k mod 4 once the pool is full), work of streams that share a queue runs in order, and a pool larger
        than 4 is time-sliced by the firmware: measured r04 (profiles/r04_hw_queues.txt) 2 / 3 / 4 / 5 / 6 / 8 queues
        give 170 / 172 / 190 / 114 / 142 / 138 img/s, and transfer streams in the high-priority pool (= more active
        queues) 140.  So the budget is four queues, and which streams share one matters."""
        mode = self.transfer_mode
        if (mode in (2, 3) and role == 'copy') or (mode == 3 and role == 'upload'):
            return main                                   # the transfers of an episode ride on its caller stream
        if (mode == 1 and role in ('upload', 'copy')) or (mode == 2 and role == 'upload'):
            key = ('xfer', 0)                             # one stream for every caller
        else:
            key = (role, main.cuda_stream)
        st = self._streams.get(key)
        if st is None:
            st = self._streams[key] = torch.cuda.Stream()
        return st

    def transfer_stream(self, mode: int = 2) -> 'torch.cuda.Stream':
        """Select a transfer arrangement and create its shared stream NOW - a serving loop calls this BEFORE it creates
        its caller streams, so that the shared stream and each of up to three caller streams get a hardware queue of
        their own.  mode 2: the result copies of an episode ride on its caller stream (no copy stream: a stream that
        waits for an episode's results blocks whatever shares its queue), one upload stream for all callers; mode 1: one
        stream for uploads AND result copies (measured r04: serialises the episodes, 190 -> 159 img/s - an upload queued
        behind a copy that waits for the previous episode holds up the next); mode 0: one upload and one copy stream
        per caller stream (round 3)."""
        self.transfer_mode = int(mode)
        return self._stream_for('upload', torch.cuda.current_stream())

    def _upload_source(self, rs: dict, dev, into: Optional[dict] = None) -> dict:
        """The source pixels of ``_source_query`` on the device, on the current stream: h_i * w_i * 3 bytes per image
        into row i of ``into['qry_src']`` (the [B, capacity] static slot of a captured graph) when that is given, else of
        a fresh buffer as wide as the largest image of the batch - what lies behind an image in its row is never read -
        and the sizes as int32 [B,2].  -> the two by name."""
        into = into or {}
        src = self._slot_rows(rs['flats'], rs['need'], rs['capacity'], dev, into.get('qry_src'))
        hw = torch.tensor(rs['sizes'], dtype=torch.int32).reshape(-1, 2)
        dhw = into.get('qry_src_hw')
        if dhw is not None and tuple(dhw.shape) == tuple(hw.shape):
            dhw.copy_(hw, non_blocking=True)
        else:
            dhw = hw.to(dev, non_blocking=True)
        return {'qry_src': src, 'qry_src_hw': dhw}

    @staticmethod
    def _device_masks(g, dev) -> torch.Tensor:
        """Ground-truth masks of one image (array or tensor) on the device as contiguous bool / uint8 [n,h,w].  Masks
        given as COCO RLE (``_gt_entries``) are decoded there (``ops.rle_decode_masks``): the same bytes, uint8 0/1, and
        only their runs cross the bus."""
        form = maskforms.form_of(g)
        if form is maskforms.COLOR:            # (made beside the upload of its image: ``_color_on_device``)
            raise ValueError('qry_isegmaps: a box + colour entry is made into a mask from its image\'s bytes, where those '
                             'are uploaded; it cannot be moved to the device on its own')
        if form is not None:                   # polygons are rasterised there: only vertices, or runs, cross the bus
            decode = ops.poly_masks if form is maskforms.POLY else ops.rle_decode_masks
            return decode(form.check(g, None, 'qry_isegmaps', None), device=dev)
        g = g if isinstance(g, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(g))
        g = g.to(dev, non_blocking=True)
        g = g if g.dtype in (torch.bool, torch.uint8) else (g != 0)
        return g.contiguous()

    @staticmethod
    def _resized_masks(g, hw, dev) -> torch.Tensor:
        """Ground-truth masks of one image on the device as bool / uint8 [n,H,W]; at another size than ``hw`` (not None)
        they are resized there (``ops.resize_masks``)."""
        g = FGN._device_masks(g, dev)
        if hw is not None and tuple(g.shape[1:]) != tuple(hw):
            g = ops.resize_masks(g, *hw)
        return g

    @staticmethod
    def _augmented_masks(g, rec: torch.Tensor, hw, dev) -> torch.Tensor:
        """Ground-truth masks of one image on the device, warped there by its record (``ops.augment_masks``): uint8
        [n,H,W]."""
        return ops.augment_masks(FGN._device_masks(g, dev), rec, *hw)

    def _upload(self, tensors: dict, gt_masks, dev, main, into: Optional[dict] = None,
                bits_out: Optional[list] = None, form: _InputForm = _InputForm()):
        """``modify_input`` (fgn.py:79-108): host -> device copies of one batch, on an upload stream so that they
        overlap the previous batch's kernels (a pinned source makes them asynchronous); the compute streams wait
        on one event.  Tensors already on the device pass through.  The ground-truth masks (copied to the GPU by
        the reference too, fgn.py:95) are run-length encoded right there (``qry_isegmaps_rle``, fgn.py:298): two
        small kernels on the upload stream instead of ~4 ms of host work per 800x1333 episode.  ``into``: device
        tensors to copy INTO (the static input buffers of a captured graph, when the upload stream is the caller
        stream itself and so ordered behind the previous replay that reads them) instead of fresh allocations.
        ``bits_out`` (``match_on_device``): a list that receives, per image, the bit planes of its ground-truth masks
        (``ops.mask_bits`` on the device copy made for the RLE, right behind it on the upload stream; None for an image
        without ground truth).  ``form.source`` (``_source_query``): the query comes at source size - its pixels go up as
        ``qry_src`` / ``qry_src_hw`` (``_upload_source``) and the masks are resized right behind their upload - unless
        ``form.at_source`` (``results_at_source``): then they are encoded and bit-packed at source size, as given.
        ``form.spp_source`` (``_source_supports``): the supports come as windows of their source images - the windows go
        up as the rows of ``spp_src`` / ``spp_msk`` (``_upload_supports``; records and boxes travel in ``tensors``)."""
        source, spp_source = form.source, form.spp_source
        gts = None
        if gt_masks is not None:
            gts = [g if isinstance(g, torch.Tensor) or maskforms.form_of(g) is not None else
                   torch.from_numpy(np.ascontiguousarray(g)) for g in gt_masks]
        colour = _has_color(gts)
        on_host = [t for t in list(tensors.values()) + (gts or []) + (source['flats'] if source else []) +
                   (spp_source['flats'] + spp_source['mflats'] if spp_source else [])
                   if t is not None and (maskforms.form_of(t) is not None or not t.is_cuda)]
        # (runs, boxes, colours and vertices are host data)
        if not on_host and gts is None and source is None:
            return tensors, None, None
        up = self._stream_for('upload', main)
        if not on_host or (colour and source is None and tensors['qry_img'].is_cuda):
            # device-resident inputs may still be being produced on the caller's stream - the image a colour mask reads too
            up.wait_stream(main)
        out, gt_out = {}, None
        with torch.cuda.stream(up):
            for k, t in tensors.items():
                if t is not None and into is not None and k in into and not t.is_cuda and into[k].dtype == t.dtype \
                        and into[k].shape == t.shape:
                    into[k].copy_(t, non_blocking=True)
                    out[k] = into[k]
                else:
                    out[k] = None if t is None else t.to(dev, non_blocking=True)
            if source is not None:
                out.update(self._upload_source(source, dev, into))
            if spp_source is not None:
                out.update(self._upload_supports(spp_source, dev, into))
            if colour:
                # box + colour entries: made from the image bytes on THIS stream, behind their copy (into a fresh buffer
                # or into the static slot of a captured graph alike) and ahead of everything that reads the masks
                slot = out['qry_src'] if source is not None else \
                    out['qry_img'].reshape(out['qry_img'].shape[0], -1)
                gts = self._color_on_device(gts, slot)
            if gts is not None:
                gt_out = []
                for g in gts:
                    g = self._resized_masks(g, source['hw'] if (source and not form.at_source) else None, dev)
                    gt_out.append(ops.dense_mask_rle(g, packed=True))
                    if bits_out is not None:
                        bits_out.append(ops.mask_bits(g) if g.shape[0] else None)
            ready = up.record_event()
        for k, t in out.items():
            if t is not None and not (into is not None and t is into.get(k)):
                t.record_stream(main)
        return out, gt_out, ready

    @torch.no_grad()
    def detect_device(self, qry_img, spp_imgs, spp_bboxes, spp_isegmaps, img_shape, support_code=None,
                      qry_isegmaps=None, phase_counter=None, qry_resize_to=None,
                      results_at_source: bool = False, spp_crop_to=None, spp_fill_ratio: float = 0.8,
                      crop_square: bool = True, spp_augment=None, spp_photometric=None, qry_bboxes=None,
                      qry_cat_ids=None, spp_photometric_chain=None) -> list:
        """Everything up to the host wait: queues the host->device copies, the whole path and the device->host
        copies of the results.  Returns, per image, a dict of device tensors (det_bboxes [D,5], det_labels [D],
        n_dets [1], mask_prob, RLE bytes) plus the pinned host slot ``pack_results`` reads.
        With ``support_code`` (from ``encode_supports``) the support branch is skipped.  ``qry_isegmaps`` (list of
        [n_i,H,W] bool): the ground-truth masks, RLE-encoded on the device for ``qry_isegmaps_rle``.  With
        ``use_graphs`` the launch sequence of one input geometry is captured once into a hipGraph and replayed
        (same kernels, same results; ~0.2 ms of host time instead of ~2 ms).  ``phase_counter``: the one-element int32
        device counter THIS call's episode bumps at ``phase_point`` (see ``_phase_mark``); passed per call, so two
        caller threads never see each other's counter (the attribute of the same name is the fallback for callers that
        set it on the model).  ``qry_resize_to``: the query comes at source size (see ``simple_test``); its pixels
        travel as ``qry_src`` (uint8 [B, slot]) and ``qry_src_hw`` (int32 [B,2]) in place of ``qry_img``, and a captured
        graph is keyed by the slot size and (H, W), not by the source sizes.  (``simple_test`` hands over the checked
        form, the dict of ``_source_query``, instead of checking twice.)  ``results_at_source`` (needs
        ``qry_resize_to``): the RLE strings, the ground-truth strings and the overlap counts are made at each image's
        source size (see ``simple_test``); the record's boxes stay in the network frame - ``pack_results`` divides them -
        and every dict carries its image's ``src_hw``.  Part of the graph key: the two modes are different launches.
        ``spp_crop_to`` = S: the supports come as their source images (see ``simple_test``); their windows travel as
        ``spp_src`` / ``spp_msk`` (uint8 [B*N*K, slot]) with the records ``spp_rec`` (int32 [B*N*K,16]) in place of
        ``spp_imgs`` / ``spp_isegmaps``, the boxes are computed on the host, and a captured graph is keyed by the slot
        size and S, not by any source, window or crop size.  (``simple_test`` hands over the dict of
        ``_source_supports``.)  Ignored beside ``support_code``.  ``spp_augment`` / ``spp_photometric`` are refused: the
        test path is without augmentation.  ``qry_bboxes`` / ``qry_cat_ids`` (per image, as ``pack_results`` will be
        given them: YXYX in the frame of the results) are read with ``evaluate_on_device`` only: the evaluator's greedy
        matching runs on the device (``ops.eval_match``) and ``pack_results`` adds the matched bits."""
        self._refuse_augment(spp_augment=spp_augment, spp_photometric=spp_photometric,
                             spp_photometric_chain=spp_photometric_chain)
        graphed = self._graphed()
        source = spp_source = None
        qry_isegmaps = self._gt_front(qry_isegmaps, qry_img, img_shape, qry_resize_to)
        if spp_crop_to is None and support_code is None:
            _dense_supports_only(spp_isegmaps)
        if spp_crop_to is not None and support_code is None:
            spp_source = spp_crop_to if isinstance(spp_crop_to, dict) else \
                self._source_supports(spp_imgs, spp_bboxes, spp_isegmaps, spp_crop_to, spp_fill_ratio, crop_square,
                                      graphed)
        results_at_source = bool(results_at_source)
        if results_at_source and qry_resize_to is None:
            raise ValueError('results_at_source needs qry_resize_to: results at source size exist for source-size queries')
        if qry_resize_to is not None:                     # (every contract error is raised here, before anything is queued)
            source = qry_resize_to if isinstance(qry_resize_to, dict) else \
                self._source_query(qry_img, qry_resize_to, img_shape, qry_isegmaps, graphed)
            img_shape = source['img_shape']
        form = _InputForm(source, spp_source, results_at_source)
        dev = self._gpu('simple_test')
        main = torch.cuda.current_stream()
        if source is None:
            self._image_dims(qry_img, 'qry_img')          # (a wrong uint8 layout is refused before anything is queued)
            ins = {'qry_img': qry_img}
        else:
            ins = {}
        if spp_source is not None:
            ins.update(spp_bboxes=spp_source['boxes'], spp_rec=spp_source['rec'])
        elif support_code is None:
            self._image_dims(spp_imgs, 'spp_imgs', lead=(1, 2))
            ins.update(spp_imgs=spp_imgs, spp_bboxes=spp_bboxes, spp_isegmaps=spp_isegmaps)
        if phase_counter is None:
            phase_counter = self.phase_counter
        # graph replay with the transfers on the caller stream: host tensors go straight into the graph's static input
        # buffers (the caller stream orders the copy behind the previous replay that reads them) - no device-to-device hop
        # (the key is taken once, ahead of the upload: that adds the slot tensors, which the key leaves out, and moves the
        # others to the device at their shapes and dtypes)
        into = key = None
        if graphed:
            key = self._graph_key(ins, img_shape, support_code, phase_counter, main, dev, form)
            if self.use_packed_transfers and self._stream_for('upload', main) is main and key in self._graphs:
                into = self._graphs[key].static
        evaluate = bool(self.evaluate_on_device)
        gt_bits = [] if ((self.match_on_device or evaluate) and qry_isegmaps is not None) else None
        ins, gt_rle, uploaded = self._upload(ins, qry_isegmaps, dev, main, into=into, bits_out=gt_bits, form=form)
        if uploaded is not None:
            main.wait_event(uploaded)
        if graphed:
            ge, outs = self._detect_graphed(ins, img_shape, support_code, phase_counter, form, key)
        else:
            outs = self._detect_eager(form.query(ins), form.supports(ins), ins.get('spp_bboxes'),
                                      ins.get('spp_isegmaps'), img_shape, support_code, phase_counter=phase_counter,
                                      results_at_source=results_at_source)
        if results_at_source:
            for d, hw in zip(outs, source['sizes']):
                d['src_hw'] = hw
        if gt_rle is not None:
            for d, g in zip(outs, gt_rle):
                d['gt_rle'] = g
        if gt_bits:
            # eager, on the caller's stream behind the network - also when the episode was a graph replay: the number of
            # ground-truth masks differs from image to image and is no part of the captured geometry (as for their RLE)
            thr = self.cfg['test_cfg']['rcnn']['mask_thr_binary']
            for d, gb in zip(outs, gt_bits):
                if gb is None:
                    continue
                for t in gb[:2]:
                    t.record_stream(main)                 # allocated on the upload stream
                if results_at_source:
                    d['overlap'] = ops.mask_overlap_src(d['mask_prob'], d['det_bboxes'], gb, d['src_hw'], d['img_hw'], thr,
                                                        d['n_dets'], skip_empty=self._skip_empty(), packed=True)[3]
                    continue
                d['overlap'] = ops.mask_overlap(d['mask_prob'], d['det_bboxes'], gb, *d['img_hw'], thr, d['n_dets'],
                                                skip_empty=self._skip_empty(), packed=True)[3]
        if evaluate and qry_bboxes is not None and qry_cat_ids is not None:
            self._match_on_device(outs, qry_bboxes, qry_cat_ids, qry_isegmaps is not None, results_at_source)
        self._start_download(outs, main, uploaded if gt_rle is not None else None)
        if graphed:
            ge.last_download = outs[0]['host_ready']
        return outs

    def _match_on_device(self, outs: list, qry_bboxes, qry_cat_ids, with_masks: bool, results_at_source: bool) -> None:
        """``evaluate_on_device``: one ``ops.eval_match`` per image on the caller's stream, right behind its overlap
        counts - eager also when the episode was a graph replay, for the reason the overlap launch gives (G is no part
        of the captured geometry).  ``with_masks``: ground-truth masks came with the call, so segm bits are made (an
        image without a ground-truth instance has no counts: every union is empty there)."""
        from .fsiseg_eval import MATCH_MAX_DETS, _xywh, gt_per_cat
        thrs = np.asarray(self.eval_iou_thrs, np.float64).reshape(-1)
        for i, d in enumerate(outs):
            if qry_bboxes[i] is None or qry_cat_ids[i] is None:
                continue
            xywh, cats = _xywh(_host(qry_bboxes[i])), _host(qry_cat_ids[i]).reshape(-1)
            md, g = d['det_bboxes'].shape[0], len(cats)
            ov = None
            if 'overlap' in d:
                o = d['overlap']
                ov = (o[:md * g].view(md, g), o[md * g:md * g + md], o[md * g + md:])
            elif with_masks and g == 0:
                z = torch.zeros(md, device=d['det_bboxes'].device, dtype=torch.int32)
                ov = (z[:0].view(md, 0), z, z[:0])
            d['match'] = ops.eval_match(d['det_bboxes'], d['det_labels'], xywh, cats, thrs, self.n_ways, overlap=ov,
                                        n_dev=d['n_dets'], max_dets=MATCH_MAX_DETS,
                                        src_hw=d['src_hw'] if results_at_source else None,
                                        net_hw=d['img_hw'] if results_at_source else None, packed=True)[2]
            d['match_meta'] = (ov is not None, thrs.copy(), gt_per_cat(cats, self.n_ways))
            d['gt_per_cat'] = torch.from_numpy(d['match_meta'][2])        # (host; ``dist.pack_matches`` sends it along)

    def _graphed(self) -> bool:
        return bool(self.use_graphs and self.debug_trace is None and ops.PROFILE is None)

    def _graph_key(self, ins: dict, img_shape, support_code, phase_counter, main, dev,
                   form: _InputForm = _InputForm()) -> tuple:
        hw = tuple((int(s[0]), int(s[1])) for s in img_shape)
        # everything the captured launch sequence depends on besides the weights (those drop ``_graphs`` when they
        # change): the paste semantic is an argument of the captured RLE kernel, the transfer arrangement decides which
        # streams the capture forks, and the phase mark is a captured kernel with the counter's address in its arguments
        self._skip_empty()
        mark = None if (phase_counter is None or not self.phase_point) else (phase_counter.data_ptr(), self.phase_point)
        return (main.cuda_stream, dev.index, hw, support_code is not None, bool(self.use_merged_backbone),
                bool(self.use_merged_support_head), self.paste_semantics, int(self.transfer_mode), mark,
                bool(self.use_side_stream), bool(self.use_packed_transfers)) + form.key(ins)

    def _detect_graphed(self, ins: dict, img_shape, support_code, phase_counter, form: _InputForm, key: tuple):
        """Replay the graph of ``key`` (``_graph_key``, taken by ``detect_device``), capturing it first where this is
        the first call of its kind."""
        ge = self._graphs.get(key)
        if ge is None:
            dev = torch.device('cuda', torch.cuda.current_device())
            ge = self._graphs[key] = _GraphedEpisode(self, ins, img_shape, support_code, dev, phase_counter, form)
        return ge, ge.run(self, ins, support_code, torch.cuda.current_stream())

    def _detect_eager(self, qry_img, spp_imgs, spp_bboxes, spp_isegmaps, img_shape, support_code=None,
                      phase_counter=None, results_at_source: bool = False) -> list:
        dev = torch.device('cuda', torch.cuda.current_device())
        if self._packed_device != dev:
            self._pack(dev)
        self._sync_trained_shared()
        with ops.arena(dev):     # zero-initialised small outputs of this episode: one fill (caller's stream only)
            return self._detect_body(qry_img, spp_imgs, spp_bboxes, spp_isegmaps, img_shape, support_code, dev,
                                     phase_counter, results_at_source)

    # Phase mark of a pipelined serving loop (bench.py): when two caller streams replay episodes side by
    # side, their relative phase settles in one of several steady states that differ by ~4 % in throughput.  A caller may
    # hand over a one-element int32 device counter (``phase_counter``) and the point of the episode at which to bump it
    # (``phase_point``: 'layer1'..'layer3' inside the backbone, 'rpn' = backbone done, 'rpn_conv', 'proposals', 'mask'):
    # ``ops.phase_signal`` is captured into the episode's
    # graph like any kernel, and the OTHER caller stream runs ``ops.phase_wait`` on that counter before its next episode.
    # (An event would be the natural tool; a captured graph cannot record one that another stream waits for on this
    # stack - "External events are disallowed in rocm".)  None: no mark.  The counter travels as an ARGUMENT of
    # ``detect_device`` (and is part of the graph cache key: a replayed graph bumps the counter it was captured with);
    # ``phase_counter`` on the model is the fallback for callers that set it there.
    phase_counter = None
    phase_point = None

    def _phase_mark(self, name: str, counter) -> None:
        if counter is not None and name == self.phase_point:
            ops.phase_signal(counter)

    def _detect_body(self, qry_img, spp_imgs, spp_bboxes, spp_isegmaps, img_shape, support_code, dev,
                     phase_counter=None, results_at_source: bool = False) -> list:
        P, cfg = self._P, self.cfg
        N, K = self.n_ways, self.k_shots
        tr = self.debug_trace
        (B,), H, W = self._image_dims(qry_img, 'qry_img')
        rh, rp, tc = cfg['roi_head'], cfg['rpn_head'], cfg['test_cfg']
        PS = rh['roi_out_size']
        inv_stride = 1.0 / rh['featmap_stride']

        qry = qry_img.to(dev, non_blocking=True)              # (dtype and layout: _stem_input)

        # Two HIP streams: the support branch (9 small crops: low-occupancy launches) runs beside
        # the query branch, and its RoI/shared-head/reduction tail runs beside the single-workgroup
        # proposal kernel.  Joined by events; no host synchronisation.
        main = torch.cuda.current_stream()
        cached = support_code is not None
        if cached:
            if support_code['B'] != B or support_code['device'] != dev:
                raise ValueError('support_code was encoded for another batch size or device')
            side = main
        elif self.use_side_stream:
            side = self._stream_for('side', main)              # one side stream per caller stream
        else:
            side = main
        merged = (not cached) and self.use_merged_backbone and self.cfg['backbone'].get('norm', 'BN') == 'BN' and \
            self.cfg['backbone'].get('block', 'bottleneck') == 'bottleneck'
        # merged shared head: rows [0, ns) of the box head's RoI batch are the support RoIs
        msh = (not cached) and self.use_merged_support_head
        ns = B * N * K
        x_all = y1_all = None
        if msh:
            c4 = rh['shared_head']['inplanes']
            x_all = torch.empty((ns + B * tc['rpn']['max_per_img'], PS, PS, c4), device=dev, dtype=torch.float32)
            if P['sh0_lin'] is not None:
                y1_all = torch.empty(tuple(x_all.shape[:3]) + (P['sh0_lin'].cout,), device=dev, dtype=torch.float32)
            if side is not main and not torch.cuda.is_current_stream_capturing():
                x_all.record_stream(side)
                if y1_all is not None:
                    y1_all.record_stream(side)

        def support_tail():       # on the side stream, right behind the support maps
            if msh:
                self._support_rois(sc, B, dev, x_all[:ns], None if y1_all is None else y1_all[:ns])
            else:
                self._support_back(sc, B, dev)
        qry_fmap = None
        if cached:
            sc = support_code
        elif merged:
            sc = self._support_front(spp_imgs, spp_bboxes, spp_isegmaps, B, dev, main, defer_backbone=True)
            qry_fmap, spp_fmaps = self.extract_feat_pair(qry, sc.pop('spp'), phase_counter)
            backbone_done = main.record_event()
            with torch.cuda.stream(side):
                side.wait_event(backbone_done)
                self._support_vectors(sc, spp_fmaps)
                vec_ready = side.record_event()
                support_tail()
            if side is not main and not torch.cuda.is_current_stream_capturing():
                spp_fmaps.record_stream(side)
        else:
            side.wait_stream(main)
            with torch.cuda.stream(side):
                sc = self._support_front(spp_imgs, spp_bboxes, spp_isegmaps, B, dev, side)
                vec_ready = side.record_event()
                # count_spp (fgn_roi_head.py:419-449) follows at once: its ~30 tiny 9-RoI launches run beside the
                # second half of the query backbone.  (Released later, at the AG-RPN conv, they were starved by that
                # conv's persistent workgroups and the RoI head waited ~0.1 ms for them.)
                support_tail()
        vec = sc['vec']

        if qry_fmap is None:
            qry_fmap = self.extract_feat(qry)                   # [B,h,w,C]
        fh, fw, C = qry_fmap.shape[1:]
        if tr is not None:
            tr['qry_fmap'], tr['spp_fmaps'] = qry_fmap, sc.get('spp_fmaps')

        # ---- AG-RPN (fgn_ag_rpn_head.py:26-118) -------------------------------------------
        if not cached:
            main.wait_event(vec_ready)
        rpn_start = main.record_event()
        self._phase_mark('rpn', phase_counter)
        # guidance multiply (fgn_ag_rpn_head.py:44): never materialised - it rides in the Winograd input transform,
        # or in the A-operand staging of the direct kernel where the layer is too small for the Winograd form
        if P['rpn_conv_wg'] is not None and ops.winograd_fits(B * N, fh, fw, C, P['rpn_conv_wg'].cout,
                                                              P['rpn_conv_wg'].m):
            # Winograd F(2x2,3x3); the guidance multiply rides in its input transform
            x = ops.conv3x3_winograd(qry_fmap, P['rpn_conv_wg'], in_scale=vec, a_img_div=N)
        else:
            x = ops.conv2d(ops.scale_channels(qry_fmap, vec, N), P['rpn_conv'])
        self._phase_mark('rpn_conv', phase_counter)
        head = ops.conv2d(x, P['rpn_head'])                                     # [B*N,h,w,5A]
        A = P['anchors'].shape[0]
        logits, scores, deltas = ops.rpn_merge(head, B, N, A)

        # ---- shared_head conv1 on the query map (see _roi_feats): independent of the proposals, so it runs on the
        # side stream beside the AG-RPN transforms and the proposal kernels instead of after them
        g_map = None
        if not cached:
            with torch.cuda.stream(side):
                if P['sh0_lin'] is not None and side is not main:
                    side.wait_event(rpn_start)
                    g_map = ops.conv2d(qry_fmap, P['sh0_lin'])
                spp_ready = side.record_event()
            if not torch.cuda.is_current_stream_capturing():
                for key in ('spp_fmaps', 'vec', 'masks7') if msh else ('spp_fmaps', 'vec', 'S', 'cat_mean', 'cat_mean_mp', 'masks7'):
                    sc[key].record_stream(main)                                   # produced on side, consumed on main
                if g_map is not None:
                    g_map.record_stream(main)
                    qry_fmap.record_stream(side)
        ih, iw = int(img_shape[0][0]), int(img_shape[0][1])
        if any(int(s[0]) != ih or int(s[1]) != iw for s in img_shape):
            raise ValueError('all images of a batch must share img_shape (the dataset batches by size)')
        props, n_props, rois_all = ops.rpn_proposals(scores, deltas, P['anchors'], fh, fw, rp['anchor_stride'], ih, iw,
                                                     rp['target_means'], rp['target_stds'], tc['rpn']['nms_pre'],
                                                     tc['rpn']['min_bbox_size'], tc['rpn']['nms_iou_threshold'],
                                                     tc['rpn']['max_per_img'], with_rois=True)   # [B*R,5] = bbox2roi
        if not cached:
            main.wait_event(spp_ready)
        if tr is not None:
            tr.update(class_vec=vec, rpn_logits=logits, rpn_scores=scores, rpn_deltas=deltas, proposals=props,
                      n_props=n_props)

        self._phase_mark('proposals', phase_counter)
        # ---- box head on the proposals of all B images at once (fgn_roi_head.py:531-616); a RoI carries its
        # image index in column 0 (bbox2roi), which selects the feature map in RoIAlign and the support set
        # in the relation head.  With one image the device-side proposal count bounds every launch; with
        # several images the valid RoIs are not a prefix of the list, so the zero-box padding rows are
        # computed too and dropped per image by det_post.
        rel, bh = rh['relation'], rh['bbox_head']
        R, D = props.shape[1], tc['rcnn']['max_per_img']
        cnt_all = n_props[0:1] if B == 1 else None
        if g_map is None and P['sh0_lin'] is not None:
            g_map = ops.conv2d(qry_fmap, P['sh0_lin'])                                # [B,h,w,planes]
        if msh:
            # support RoIs (pooled on the side stream) and proposals through the shared head as ONE RoI batch
            inv = 1.0 / rh['featmap_stride']
            ops.roi_align(qry_fmap, rois_all, PS, inv, rh['roi_sampling_ratio'], True, cnt_all, out=x_all[ns:])
            if y1_all is not None:
                ops.roi_align(g_map, rois_all, PS, inv, rh['roi_sampling_ratio'], True, cnt_all,
                              post_shift=P['sh0_shift'], relu=True, out=y1_all[ns:])
            cnt_plus = None if cnt_all is None else cnt_all + ns
            feats_all = self._shared_head(x_all, cnt_plus, y1=y1_all)
            self._support_finish(sc, feats_all[:ns], B)
            feats = feats_all[ns:]
        else:
            _, feats = self._roi_feats(qry_fmap, g_map, rois_all, cnt_all)
        S, cat_mean, cat_mean_mp, masks7 = sc['S'], sc['cat_mean'], sc['cat_mean_mp'], sc['masks7']
        if tr is not None:
            tr.update(spp_masks7=masks7, spp_cat_mean=cat_mean, spp_cat_mean_mp=cat_mean_mp)
        Q = ops.conv2d(feats, P['rel_q'], n_img_dev=cnt_all)
        cls_raw, reg_raw = ops.relation_gn_head(Q, S, rois_all, P['gn_w'], P['gn_b'], P['fc_w'], P['fc_b'], N,
                                                rel['gn_groups'], rel['gn_eps'], cnt_all)
        # the batch's result record: detections, labels, counts, mask probabilities and RLE strings land in one buffer
        rec = _ResultRecord(B, D, 2 * PS, dev)
        rec.clear_head()
        packed = self.use_packed_transfers
        # one selection workgroup per image, one launch for the batch
        det_all, lab_all, n_det_all, mrois_all = ops.det_post(
            rois_all, cls_raw, reg_raw, N, ih, iw, bh['target_means'], bh['target_stds'], tc['rcnn']['score_thr'],
            tc['rcnn']['nms_iou_threshold'], D, n_props, img_index=0, batch=B,
            out=(rec.det.view(B * D, 5), rec.lab.view(B * D), rec.cnt.view(B)))      # mrois_all [B*D,5] = bbox2roi
        dets = [det_all[i * D:(i + 1) * D] for i in range(B)]
        labs = [lab_all[i * D:(i + 1) * D] for i in range(B)]
        n_dets = [n_det_all[i:i + 1] for i in range(B)]
        self._phase_mark('mask', phase_counter)
        # ---- mask head on the detections of all images at once (fgn_roi_head.py:704-718, 360-382)
        nd_all = n_dets[0] if B == 1 else None
        vmask = ops.gather_support_vectors(cat_mean_mp, lab_all, mrois_all, N, nd_all)
        _, mf = self._roi_feats(qry_fmap, g_map, mrois_all, nd_all)
        mlog, mprob = self._mask_head(mf, vmask, nd_all, prob_out=rec.prob.view(B * D, 2 * PS, 2 * PS))
        outs = []
        skip_empty = self._skip_empty()
        src_boxes = src_sizes = None
        if results_at_source:
            # results at source size: ONE launch for the batch, the images' sizes read from ``qry_src_hw``
            # on the device - the launch is the same for every source size, so a captured graph serves them all
            if getattr(qry, 'hw', None) is None:
                raise ValueError('results_at_source needs a source-size query (qry_resize_to)')
            if tr is not None:                  # (a trace is never captured: the host may read the sizes)
                src_boxes = torch.empty((B * D, 4), device=dev, dtype=torch.float32)
                src_sizes = qry.hw.cpu().tolist()
            ops.mask_rle_src(mprob, det_all, qry.hw, (ih, iw), tc['rcnn']['mask_thr_binary'], n_det_all,
                             skip_empty=skip_empty, boxes_src_out=src_boxes,
                             out=(rec.rle.view(B * D, -1), rec.rle_len.view(B * D), rec.rle_ovf.view(B * D)))
        for i in range(B):
            det, lab, n_det = dets[i], labs[i], n_dets[i]
            mp_i = mprob[i * D:(i + 1) * D]
            if results_at_source:
                rle_bytes, rle_len, rle_ovf = rec.rle[i], rec.rle_len[i], rec.rle_ovf[i]
            else:
                # paste + threshold + COCO RLE fused on device: the D x H x W masks are never written
                rle_bytes, rle_len, rle_ovf = ops.mask_rle(mp_i, det, ih, iw, tc['rcnn']['mask_thr_binary'], n_det,
                                                           skip_empty=skip_empty,
                                                           out=(rec.rle[i], rec.rle_len[i], rec.rle_ovf[i]))
            if tr is not None:
                if results_at_source:
                    masks = ops.mask_paste(mp_i, src_boxes[i * D:(i + 1) * D], *src_sizes[i],
                                           tc['rcnn']['mask_thr_binary'], n_det, skip_empty=skip_empty)
                else:
                    masks = ops.mask_paste(mp_i, det, ih, iw, tc['rcnn']['mask_thr_binary'], n_det, skip_empty=skip_empty)
                tr.setdefault('per_image', []).append(dict(
                    rois=rois_all[i * R:(i + 1) * R], roi_feats=feats[i * R:(i + 1) * R], Q=Q[i * R:(i + 1) * R],
                    cls_raw=cls_raw[i * R * N:(i + 1) * R * N], reg_raw=reg_raw[i * R * N:(i + 1) * R * N],
                    det=det, lab=lab, n_det=n_det, mask_logits=mlog[i * D:(i + 1) * D], mask_prob=mp_i,
                    masks=masks, mask_feats=mf[i * D:(i + 1) * D]))
            outs.append(dict(det_bboxes=det, det_labels=lab, n_dets=n_det, mask_prob=mp_i, rle_bytes=rle_bytes,
                             rle_len=rle_len, rle_overflow=rle_ovf, img_hw=(ih, iw), record=rec if packed else None))
        return outs

    MAX_SLOTS = 64

    def _pinned_slot(self, batch: int, max_det: int, n_gt: int, mask_size: int = 14, n_ov: int = 0,
                     with_match: bool = False) -> dict:
        """A free pinned host slot for one batch's results (pinned allocation is slow, so slots are kept per
        (batch, max_det, mask size) and reused): the host mirror of a ``_ResultRecord`` plus a byte buffer for the
        packed ground-truth RLE.  A slot is busy from ``detect_device`` until ``pack_results`` has read it; when every
        slot is busy (more batches in flight than ever before) another one is allocated."""
        key = (batch, max_det, mask_size, ops.RLE_BYTE_CAP)
        ring = self._pinned.setdefault(key, [])
        slot = next((s for s in ring if not s['busy']), None)
        if slot is None:
            if len(ring) >= self.MAX_SLOTS:
                raise ops._lib.FgnHipError(f'{self.MAX_SLOTS} batches are in flight without pack_results(); '
                                           'pack (or drop and call release_results on) earlier detect_device outputs')
            rec = _ResultRecord(batch, max_det, mask_size, pinned=True)
            slot = dict(key=key, busy=False, gt_cap=0, rec=rec, det=rec.det, lab=rec.lab, cnt=rec.cnt, rle_len=rec.rle_len,
                        rle_ovf=rec.rle_ovf, rle=rec.rle, prob=rec.prob)
            ring.append(slot)
        if n_gt > slot['gt_cap']:
            # generous from the start: growing a slot is a pinned allocation (~5 ms of host time) in the middle of a
            # pipelined run - with caps of 2 x the first count seen, slots kept growing for dozens of steps
            cap = max(64, 2 * n_gt)
            slot.update(gt_cap=cap, gt_buf=torch.empty(cap * (ops.RLE_BYTE_CAP + 8), dtype=torch.uint8, pin_memory=True))
        if n_ov > slot.get('ov_cap', 0):
            # overlap counts (``match_on_device``), grown like gt_buf: n_ov ground-truth masks take at most
            # n_ov * (max_det + 1) + batch * max_det int32 ([inter | det_area | gt_area] per image)
            cap = max(64, 2 * n_ov)
            slot.update(ov_cap=cap, ov_buf=torch.empty(cap * (max_det + 1) + batch * max_det, dtype=torch.int32,
                                                       pin_memory=True))
        if with_match and 'mt_buf' not in slot:
            # matched bits (``evaluate_on_device``): [bbox | segm] rows of max_det int32 per image - a fixed size
            slot['mt_buf'] = torch.empty(batch * 2 * max_det, dtype=torch.int32, pin_memory=True)
        slot['busy'] = True
        return slot

    @staticmethod
    def release_results(dets: list) -> None:
        """Give back the pinned host slot of ``detect_device`` outputs that will not be packed."""
        if dets and 'host' in dets[0]:
            dets[0]['host']['busy'] = False

    def _start_download(self, outs: list, main, also_wait=None) -> None:
        """Queue the device->host copies of one batch on a copy stream behind the compute work;
        ``pack_results`` later waits on the event only, so the next batch's kernels are not
        serialised behind a host round trip."""
        cp = self._stream_for('copy', main)
        max_det = outs[0]['det_bboxes'].shape[0]
        n_gt = sum(d['gt_rle'][1].shape[0] for d in outs if 'gt_rle' in d)
        rec = outs[0].get('record')
        n_ov = sum(d['gt_rle'][1].shape[0] for d in outs if 'overlap' in d)
        slot = self._pinned_slot(len(outs), max_det, n_gt, outs[0]['mask_prob'].shape[-1], n_ov,
                                 any('match' in d for d in outs))
        cp.wait_stream(main)
        if also_wait is not None:
            cp.wait_event(also_wait)           # the ground-truth RLE kernels run on the upload stream
        with torch.cuda.stream(cp):
            if rec is not None and rec.key == slot['rec'].key:
                # ONE copy for the batch: detections, labels, counts, RLE strings and lengths, mask probabilities
                slot['rec'].buf.copy_(rec.buf, non_blocking=True)
                rec.buf.record_stream(cp)
            else:                  # outputs assembled by hand (tests): field by field
                for i, d in enumerate(outs):
                    for dst, src in (('det', 'det_bboxes'), ('lab', 'det_labels'), ('cnt', 'n_dets'), ('rle_len', 'rle_len'),
                                     ('rle_ovf', 'rle_overflow'), ('rle', 'rle_bytes'), ('prob', 'mask_prob')):
                        slot[dst][i].copy_(d[src].reshape(slot[dst][i].shape), non_blocking=True)
                        d[src].record_stream(cp)
            g0 = 0
            row = ops.RLE_BYTE_CAP + 8
            for d in outs:
                if 'gt_rle' in d:
                    n = d['gt_rle'][1].shape[0]
                    if n:
                        if len(d['gt_rle']) == 4:        # packed [lens | overflow | bytes]: one copy per image
                            slot['gt_buf'][g0 * row:(g0 + n) * row].copy_(d['gt_rle'][3], non_blocking=True)
                            d['gt_rle'][3].record_stream(cp)
                        else:
                            hb = slot['gt_buf'][g0 * row:(g0 + n) * row]
                            gb, gl, go = d['gt_rle'][:3]
                            hb[:n * 4].view(torch.int32).copy_(gl, non_blocking=True)
                            hb[n * 4:n * 8].view(torch.int32).copy_(go, non_blocking=True)
                            hb[n * 8:].view(n, ops.RLE_BYTE_CAP).copy_(gb, non_blocking=True)
                            for t in (gb, gl, go):
                                t.record_stream(cp)
                    d['gt_slice'] = (g0, n)
                    g0 += n
            o0 = 0
            for d in outs:
                if 'overlap' in d:
                    n = d['overlap'].numel()
                    slot['ov_buf'][o0:o0 + n].copy_(d['overlap'], non_blocking=True)
                    d['overlap'].record_stream(cp)
                    d['ov_slice'] = (o0, n)
                    o0 += n
            for i, d in enumerate(outs):
                if 'match' in d:                   # the matched bits, in a slice of their own
                    n = d['match'].numel()
                    slot['mt_buf'][i * n:(i + 1) * n].copy_(d['match'].reshape(-1), non_blocking=True)
                    d['match'].record_stream(cp)
                    d['mt_slice'] = (i * n, n)
            ev = cp.record_event()
        for d in outs:
            d['host'] = slot
            d['host_ready'] = ev

    def pack_results(self, dets: list, batch: int, qry_bboxes=None, qry_cat_ids=None, qry_isegmaps=None,
                     img_shape=None, qry_child_idx=None, cats_ids_to_sample_real=None, spp_insts_ids=None,
                     idx=None, qry_resize_to=None, results_at_source: bool = False) -> List[Dict]:
        """Device->host copy and result dicts (fgn.py:240-303).  Passthrough boxes stay YXYX
        (SERVER semantics); caller tensors are never mutated.  ``qry_resize_to`` = (H, W):
        ``qry_isegmaps`` are at source size (they are read only where a device RLE overflowed or none was made, and
        resized on the host then).  ``results_at_source``: ``dets`` come from ``detect_device`` with the same flag
        and carry each image's (h_b, w_b), checked by ``_source_query``: boxes are divided by the image's scale
        (``fewshot_ds.boxes_to_source``), strings carry ``size: [h_b, w_b]``, ``qry_img_shape`` is ``[h_b, w_b, 3]``
        and no mask is resized."""
        from .fewshot_ds import boxes_to_source
        if results_at_source and any('src_hw' not in d for d in dets[:batch]):
            raise ValueError('results_at_source: these detections were not made with detect_device(results_at_source=True)')

        def host_mask(m):
            m = maskforms.dense(m, 'qry_isegmaps')      # a compact form: decoded, rasterised or derived on the host here only
            m = np.asarray(m.cpu() if isinstance(m, torch.Tensor) else m)
            if results_at_source:               # as given
                return m
            if qry_resize_to is not None and tuple(m.shape[-2:]) != tuple(qry_resize_to):
                from .fewshot_ds import resize_masks
                m = resize_masks(m.reshape((-1,) + m.shape[-2:]), *qry_resize_to).reshape(m.shape[:-2] + tuple(qry_resize_to))
            return m
        passthrough = {'idx': idx, 'qry_bboxes': qry_bboxes, 'qry_img_shape': img_shape,
                       'qry_cat_ids': qry_cat_ids, 'qry_child_idx': qry_child_idx,
                       'cats_ids_to_sample_real': cats_ids_to_sample_real, 'spp_insts_ids': spp_insts_ids}
        dets[0]['host_ready'].synchronize()        # the one host wait: the batch's D2H copies
        host = dets[0]['host']
        results = []
        for i in range(batch):
            di = dets[i]
            n = int(host['cnt'][i, 0])
            db = host['det'][i, :n].numpy()
            lens = host['rle_len'][i, :n].numpy()
            ovf = host['rle_ovf'][i, :n].numpy()
            ih, iw = di['img_hw']
            oh, ow = di['src_hw'] if results_at_source else (ih, iw)        # the frame of this image's results
            strings = host['rle'][i].numpy()
            rles = [{'size': [oh, ow], 'counts': strings[j, :lens[j]].tobytes()} for j in range(n)]
            if n and ovf.any():     # a device cap overflowed: dense paste + host RLE for those masks only
                thr = self.cfg['test_cfg']['rcnn']['mask_thr_binary']
                for j in np.flatnonzero(ovf):
                    # (from the HOST copies: a replayed graph may have overwritten the device tensors by now)
                    pdev = di['det_bboxes'].device
                    box = host['det'][i, j:j + 1]
                    if results_at_source:       # the box the device divided, divided here by the same rule
                        box = torch.from_numpy(boxes_to_source(np.ascontiguousarray(box[:, :4].numpy()), (oh, ow),
                                                               (ih, iw), order='xyxy'))
                    dense = ops.mask_paste(host['prob'][i, j:j + 1].to(pdev).contiguous(), box.to(pdev).contiguous(),
                                           oh, ow, thr, skip_empty=self._skip_empty())
                    rles[j] = rle.encode(dense[0].cpu().numpy())
            boxes = db[:, [1, 0, 3, 2]].reshape(-1, 4).copy()
            if results_at_source:
                boxes = boxes_to_source(boxes, (oh, ow), (ih, iw), order='yxyx')
            one = {'dt_scores': db[:, 4].reshape(-1).copy(),
                   'dt_bboxes': boxes,
                   'dt_cat_ids': host['lab'][i, :n].numpy().copy().reshape(-1),
                   'dt_isegmaps_rle': rles}
            for key, val in passthrough.items():
                v = val[i] if val is not None else None
                one[key] = v.cpu().numpy() if isinstance(v, torch.Tensor) else v
            if results_at_source:
                sh = one['qry_img_shape']
                one['qry_img_shape'] = np.array([oh, ow, 3], sh.dtype if isinstance(sh, np.ndarray) else np.int32)
            gt = qry_isegmaps[i] if qry_isegmaps is not None else None
            if 'gt_slice' in di:                   # ground-truth masks were encoded on the device (detect_device)
                g0, ng = di['gt_slice']
                row = ops.RLE_BYTE_CAP + 8
                hb = host['gt_buf'][g0 * row:(g0 + ng) * row]
                glen, govf = hb[:ng * 4].view(torch.int32).numpy(), hb[ng * 4:ng * 8].view(torch.int32).numpy()
                gstr = hb[ng * 8:].view(ng, ops.RLE_BYTE_CAP).numpy()
                on_host = host_mask(gt) if govf.any() else None     # (once, for the masks whose device RLE overflowed)
                one['qry_isegmaps_rle'] = [
                    {'size': [oh, ow], 'counts': gstr[j, :glen[j]].tobytes()} if not govf[j] else
                    rle.encode(on_host[j])
                    for j in range(ng)]
            elif gt is not None:
                one['qry_isegmaps_rle'] = rle.encode_many(host_mask(gt)) if len(gt) else []
            if 'ov_slice' in di:                   # overlap counts from the device: [inter [D,G] | det_area [D] | gt_area [G]]
                o0, nov = di['ov_slice']
                md = host['det'].shape[1]
                ng = (nov - md) // (md + 1)
                hb = host['ov_buf'][o0:o0 + nov].numpy()
                one['dt_gt_inter'] = hb[:md * ng].reshape(md, ng)[:n].copy()
                one['dt_area'] = hb[md * ng:md * ng + md][:n].copy()
                one['gt_area'] = hb[md * ng + md:].copy()
            if 'mt_slice' in di:                   # matched bits from the device: [bbox [D] | segm [D]]
                m0, nm = di['mt_slice']
                fl = host['mt_buf'][m0:m0 + nm].numpy().reshape(2, -1)
                has_segm, thrs, per_cat = di['match_meta']
                one['dt_match_bbox'] = fl[0, :n].copy()
                if has_segm:
                    one['dt_match_segm'] = fl[1, :n].copy()
                one['eval_iou_thrs'] = thrs
                one['gt_per_cat'] = per_cat
            results.append(one)
        host['busy'] = False
        return results
