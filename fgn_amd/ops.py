"""Thin tensor-level wrappers over the C-ABI (fgn_amd.lib).

PyTorch is plumbing here: it owns device memory and the HIP stream; every op validates
operand shapes on the host (a mis-shaped launch can fault the GPU), passes raw device
pointers plus the current stream to libfgn_hip.so, and raises on any error.  Tensors
are NHWC fp32 and must be contiguous.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import lib as _lib


# Live HIP-event timing of the convolution launches (bench.py roofline): when set to a ConvProfile, every conv
# launch appends a record dict(kind, kernel, e0, e1, flop_direct, flop_issued, n_img, n_img_dev, shape):
#   kind        'conv' (one fgn_conv2d launch, incl. its split-K reduce), 'wg_in' / 'wg_gemm' / 'wg_out' (the three
#               kernels of a Winograd layer, bracketed separately)
#   kernel      name of the device kernel as rocprofv3 reports it (from fgn_conv2d_kernel_id)
#   flop_*      per image: direct-convolution FLOPs of the layer / MFMA FLOPs actually issued (0 for the transforms)
PROFILE = None

# conv3 + shortcut conv of the first block of a stride-1 stage as one dual-operand K loop (conv1x1_dual).  A/B knob.
FUSED_SHORTCUT = os.environ.get('FGN_FUSED_SHORTCUT', '1') != '0'
# Arithmetic of the GEMM-shaped launches (1x1 / stride 1 convolutions, the fused conv3 + shortcut, the Winograd GEMMs):
# 'x3' = conv_pw_x3_kernel, every f32 product as six bf16 MFMA products of exact three-way splits, f32 accumulation
# (csrc/conv_pw_x3.h; the packers below then also build the weights' bf16-plane image); 'f32' = the f32-input MFMA kernels;
# 'h2' (default) = conv_pw_h2_kernel: three f16 MFMA products of two-way splits of the power-of-two scaled operands per f32
# product (csrc/conv_pw_h2.h; the packers then build the weights' f16-plane image instead), on the same launches.
GEMM_MATH = os.environ.get('FGN_GEMM_MATH', 'h2')
# by row tile (fgn_x3_row_tile); template arguments: waves along M, 32-row blocks per wave, terms, LDS stages, 16x16x32 MFMA
X3_KERNELS = {64: 'conv_pw_x3_kernel<2, 1, 6, 2, true>', 128: 'conv_pw_x3_kernel<2, 2, 6, 2, true>'}
# by tile (fgn_h2_row_tile: 64 / 128 rows x 128 columns, 264 = 128 rows x 64 columns); template arguments: waves along M,
# waves along N, 32-row blocks per wave, LDS stages, implicit-GEMM loader (3x3 / strided convolutions), K-groups;
# 1064 = the 64-row tile on two K-groups (fgn_h2_k_groups; also the forced tile code of gemm_h2 / conv2d_pair)
H2_KERNELS = {64: 'conv_pw_h2_kernel<2, 2, 1, 2, %s, 1>', 128: 'conv_pw_h2_kernel<2, 2, 2, 2, %s, 1>',
              264: 'conv_pw_h2_kernel<4, 1, 1, 2, %s, 1>', 1064: 'conv_pw_h2_kernel<2, 2, 1, 2, %s, 2>'}
H2_BM_KG2 = 1064
# the instances of the launches with a second operand (conv1x1_dual), by the same tile codes; template arguments: waves
# along M, waves along N, 32-row blocks per wave, LDS stages, K-groups
H2_DUAL_KERNELS = {64: 'conv_pw_h2_kernel_dual<2, 2, 1, 2, 1>', 128: 'conv_pw_h2_kernel_dual<2, 2, 2, 2, 1>',
                   264: 'conv_pw_h2_kernel_dual<4, 1, 1, 2, 1>', 1064: 'conv_pw_h2_kernel_dual<2, 2, 1, 2, 2>'}


def x3_kernel(rows: int, cout: int, k: int, grp_rows: int = 0, grp_valid: int = 0) -> str:
    """Name (as rocprofv3 reports it) of the conv_pw_x3_kernel instance a GEMM of this shape is launched on."""
    return X3_KERNELS.get(_lib.load().fgn_x3_row_tile(rows, cout, k, grp_rows, grp_valid), 'conv_pw_x3_kernel<?>')


def h2_kernel(rows: int, cout: int, k: int, grp_rows: int = 0, grp_valid: int = 0, im2col: bool = False) -> str:
    """The same for conv_pw_h2_kernel (the instance a launch with nothing forced runs on: tile and K-groups)."""
    L = _lib.load()
    tile = L.fgn_h2_row_tile(rows, cout, k, grp_rows, grp_valid)
    if tile == 64 and L.fgn_h2_k_groups(rows, cout, k, grp_rows, grp_valid) == 2:
        tile = H2_BM_KG2
    return H2_KERNELS.get(tile, 'conv_pw_h2_kernel<?, %s>') % ('true' if im2col else 'false')


def h2_dual_kernel(rows: int, cout: int, k: int, bm: int = 0) -> str:
    """The conv_pw_h2_kernel_dual instance a two-operand launch of this shape runs on (``bm``: a forced tile code)."""
    L = _lib.load()
    tile = bm
    if tile == 0:
        tile = L.fgn_h2_row_tile(rows, cout, k, 0, 0)
        if tile == 64 and L.fgn_h2_k_groups(rows, cout, k, 0, 0) == 2:
            tile = H2_BM_KG2
    return H2_DUAL_KERNELS.get(tile, 'conv_pw_h2_kernel_dual<?>')


class gemm_math:
    """``with ops.gemm_math('f32'):`` - the layers PACKED inside use that arithmetic (None: no change).  Training packs its
    head layers under 'f32': the optimizer rewrites their weights in place every step and a plane image would have to
    be re-derived each time."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        global GEMM_MATH
        self.prev = GEMM_MATH
        if self.mode is not None:
            GEMM_MATH = self.mode
        return self

    def __exit__(self, *exc):
        global GEMM_MATH
        GEMM_MATH = self.prev
        return False
FUSED_SHORTCUT_STRIDES = tuple(int(v) for v in os.environ.get('FGN_FUSED_SHORTCUT_STRIDES', '1,2').split(','))

_TILES = {1: (128, 128, 64, 64, 2), 2: (64, 128, 32, 64, 3), 3: (128, 64, 64, 32, 3), 4: (64, 64, 32, 32, 4)}


def kernel_name(kid: int) -> str:
    """fgn_conv2d_kernel_id -> the kernel name in a rocprofv3 kernel trace."""
    mode = kid % 10
    bm, bn, wm, wn, mw = _TILES[kid // 10]
    if mode == 4:
        return 'conv_pw_persist_kernel'
    if mode == 3:
        return f'conv_igemm_kernel<{bm}, {bn}, {wm}, {wn}, *, {mw}>'
    return f'conv_igemm_dma_kernel<{bm}, {bn}, {wm}, {wn}, 2, {mw}, {mode}>'


# route (arithmetic) of a GEMM-shaped launch -> its entry point: fgn_conv1x1_[dual_]<infix>nhwc_f32, fgn_winograd_gemm_<infix>f32
_ROUTE_INFIX = {'h2': 'h2_', 'x3': 'x3_', 'f32': ''}


def _gemm_route(L, w3, wh, rows: int, cout: int, k: int, grp_rows: int = 0, grp_valid: int = 0) -> str:
    """Route of a GEMM-shaped launch of a layer with the weight images ``w3`` (pack_x3) / ``wh`` (pack_h2) or None: that of
    the image it carries (h2 first) if that kernel's tile rule takes the shape, else 'f32'.  Preconditions: the caller's."""
    if wh is not None:
        return 'h2' if L.fgn_h2_row_tile(rows, cout, k, grp_rows, grp_valid) > 0 else 'f32'
    if w3 is not None:
        return 'x3' if L.fgn_x3_row_tile(rows, cout, k, grp_rows, grp_valid) > 0 else 'f32'
    return 'f32'


def _gemm_kernel(route: str, f32_kernel: Optional[str], *gemm) -> str:
    """Kernel name of a GEMM record by route (``gemm``: rows, cout, k[, grp_rows, grp_valid]; ``f32_kernel``: on 'f32')."""
    return f32_kernel if route == 'f32' else (h2_kernel if route == 'h2' else x3_kernel)(*gemm)


class ZeroArena:
    """One zero-filled allocation per episode from which the small zero-initialised outputs of the selection
    / head kernels are carved (counters, logits of RoIs beyond the device count, ...): one fill kernel
    instead of about ten 5 us ones on the critical path.  Opened with ``ops.arena``."""

    def __init__(self, device, nbytes: int = 2 << 20):
        self.buf = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        self.off = 0

    def take(self, shape, dtype):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        start = (self.off + 255) // 256 * 256
        if start + n > self.buf.numel():
            return None
        self.off = start + n
        return self.buf[start:start + n].view(dtype).view(*shape)


_ARENA: Optional[ZeroArena] = None


class arena:
    """``with ops.arena(device):`` - the zero arena of one episode; closed on every exit path, so an error raised
    mid-episode cannot leave a stale arena (allocated on another stream) for later ``ops.zeros`` callers.  Arenas do
    not nest and belong to one caller thread (the detector is single-caller, as the reference's is)."""

    def __init__(self, device):
        self.device = device

    def __enter__(self):
        global _ARENA
        if _ARENA is not None:
            raise _lib.FgnHipError('ops.arena: an episode is already being queued in this process')
        _ARENA = ZeroArena(self.device)
        return _ARENA

    def __exit__(self, *exc):
        global _ARENA
        _ARENA = None
        return False


def zeros(shape, device, dtype=torch.float32) -> torch.Tensor:
    """torch.zeros, served from the episode's arena when one is open on this device."""
    a = _ARENA
    if a is not None and a.buf.device == torch.device(device):
        t = a.take(tuple(shape), dtype)
        if t is not None:
            return t
    return torch.zeros(tuple(shape), device=device, dtype=dtype)


class ConvProfile(list):
    """Record list for the ``PROFILE`` hook with a pool of pre-created timing events: creating HIP
    timing events inside a timed region stalls now and then (tens of ms when the runtime grows its
    event pool), so a benchmark creates them up front with ``reserve``."""

    def __init__(self):
        super().__init__()
        self.pool = []

    def reserve(self, n_events: int):
        self.pool.extend(torch.cuda.Event(enable_timing=True) for _ in range(n_events))
        return self

    def event(self):
        """A timing event recorded on the current stream."""
        e = self.pool.pop() if self.pool else torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def arm(self):
        """Arm the library so that the next convolution-family kernel launched by this thread stamps a fresh
        (start, stop) event pair with its own start and end (fgn_profile_next_launch)."""
        pair = []
        for _ in range(2):
            if self.pool:
                pair.append(self.pool.pop())        # pool events have been recorded once: their handles exist
            else:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                pair.append(e)
        _lib.check(_lib.load().fgn_profile_next_launch(pair[0].cuda_event, pair[1].cuda_event), 'fgn_profile_next_launch')
        return pair


# ---- launch records of the dominant kernel that work inside a replayed hipGraph (include/fgn_hip.h: fgn_profile_stamps) ----
def new_stamp_records(capacity: int, device) -> torch.Tensor:
    """``capacity`` launch records (fgn_profile_stamp_words() x uint64 each, held as int64): {start, sum, shards arrived,
    executions, shortest, longest, ...}."""
    t = torch.zeros((capacity, _lib.load().fgn_profile_stamp_words()), dtype=torch.int64, device=device)
    t[:, 4] = -1
    return t


def arm_stamps(records: Optional[torch.Tensor]) -> int:
    """Arm (or, with None, disarm) the calling thread: every launch of conv_pw_persist_kernel takes the next record.
    Returns the number of records handed out since the previous call."""
    if records is None:
        return int(_lib.load().fgn_profile_stamps(None, 0))
    _chk(records, 'records', torch.int64)
    if records.dim() != 2 or records.shape[1] != _lib.load().fgn_profile_stamp_words():
        raise _lib.FgnHipError('arm_stamps: records must be [capacity, fgn_profile_stamp_words()] int64')
    return int(_lib.load().fgn_profile_stamps(_ptr(records), records.shape[0]))


def reset_stamps(records: torch.Tensor) -> None:
    """Forget the executions recorded so far (call with no launch of the graph in flight)."""
    records[:, 1] = 0
    records[:, 3] = 0
    records[:, 4] = -1
    records[:, 5] = 0


def read_stamps(records: torch.Tensor, n: int) -> list:
    """[{executions, total_us, min_us, max_us}] of the first ``n`` records (10 ns ticks -> microseconds)."""
    r = records[:n].cpu().numpy().view(np.uint64)
    return [dict(executions=int(x[3]), total_us=float(x[1]) * 0.01,
                 min_us=(float(x[4]) * 0.01 if x[3] else None), max_us=(float(x[5]) * 0.01 if x[3] else None)) for x in r]


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def phase_signal(counter: torch.Tensor) -> None:
    """Bump the int32 device counter from the current stream (inside a captured graph: on every replay)."""
    _chk(counter, 'counter', torch.int32)
    _lib.check(_lib.load().fgn_phase_signal(_ptr(counter), _stream()), 'fgn_phase_signal')


def phase_wait(counter: torch.Tensor, target: int, timeout_us: int = 50000) -> None:
    """Hold the current stream until the counter has reached ``target`` (or the timeout has passed)."""
    _chk(counter, 'counter', torch.int32)
    _lib.check(_lib.load().fgn_phase_wait(_ptr(counter), int(target), int(timeout_us), _stream()), 'fgn_phase_wait')


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _chk(t: torch.Tensor, name: str, dtype=torch.float32):
    if not t.is_cuda:
        raise _lib.FgnHipError(f'{name} must be a device tensor (no CPU fallback)')
    if t.dtype != dtype:
        raise _lib.FgnHipError(f'{name} must be {dtype}, got {t.dtype}')
    if not t.is_contiguous():
        raise _lib.FgnHipError(f'{name} must be contiguous')


def _f4(vals):
    return (C.c_float * 4)(*[float(v) for v in vals])


# --------------------------------------------------------------------------------------
# convolution
# --------------------------------------------------------------------------------------
@dataclass
class ConvLayer:
    """A packed convolution: weights [cout_pad, KH*KW*Cin (padded to x32)], folded
    per-channel epilogue scale/shift (eval-mode BN or bias)."""
    w: torch.Tensor
    scale: Optional[torch.Tensor]
    shift: Optional[torch.Tensor]
    cin: int
    cout: int
    cout_pad: int
    kh: int
    kw: int
    stride: int
    pad: int
    relu: bool
    w3: Optional[torch.Tensor] = None      # bf16-plane image of w (pack_x3) for conv_pw_x3_kernel, or None
    wh: Optional[torch.Tensor] = None      # f16-plane image of w (pack_h2) for conv_pw_h2_kernel, or None

    def to(self, device):
        self.w = self.w.to(device)
        self.scale = None if self.scale is None else self.scale.to(device)
        self.shift = None if self.shift is None else self.shift.to(device)
        self.w3 = None if self.w3 is None else self.w3.to(device)
        self.wh = None if self.wh is None else self.wh.to(device)
        return self


def _x3_ok(cin: int, cout: int) -> bool:
    """Whether a layer gets a bf16-plane image: the shapes conv_pw_x3_kernel takes and wins on (fgn_x3_row_tile decides per
    launch; a layer whose 128-column tiles would be under 70 % real channels never passes it)."""
    npad = (cout + 127) // 128 * 128
    return GEMM_MATH == 'x3' and cin % 32 == 0 and cin >= 64 and cout % 4 == 0 and cout * 10 >= npad * 7


def _h2_ok(cin: int, cout: int) -> bool:
    """The same for the f16-plane image of conv_pw_h2_kernel (GEMM_MATH 'h2': the launches 'x3' would take, and - on its
    64-column tile - layers of 48 .. 64 output channels; fgn_h2_row_tile decides per launch)."""
    npad = (cout + 127) // 128 * 128
    return GEMM_MATH == 'h2' and cin % 32 == 0 and cin >= 64 and cout % 4 == 0 and (cout * 10 >= npad * 7 or 48 <= cout <= 64)


def _h2_conv_ok(cin: int, cout: int, kh: int, kw: int) -> bool:
    """Whether a 3x3 (any stride) or strided 1x1 convolution gets an f16-plane image for the implicit-GEMM form of
    conv_pw_h2_kernel (fgn_conv2d_pair_h2_nhwc_f32): Cin / 32 a power of two."""
    ct = cin // 32
    return _h2_ok(cin, cout) and (kh, kw) in ((1, 1), (3, 3)) and ct & (ct - 1) == 0


def pack_conv(weight: torch.Tensor, bias: Optional[torch.Tensor] = None, bn: Optional[dict] = None,
              stride: int = 1, pad: int = 0, relu: bool = False, eps: float = 1e-5,
              pad_cin_to: Optional[int] = None) -> ConvLayer:
    """weight [Cout,Cin,KH,KW] (torch layout) -> ConvLayer.  ``bn`` = dict(weight, bias,
    running_mean, running_var) folds eval-mode BatchNorm into scale/shift."""
    weight = weight.detach().float()
    cout, cin, kh, kw = weight.shape
    if pad_cin_to is not None and pad_cin_to > cin:
        weight = torch.cat([weight, weight.new_zeros(cout, pad_cin_to - cin, kh, kw)], dim=1)
        cin = pad_cin_to
    cout_pad = (cout + 127) // 128 * 128
    if cin == 4:
        # stem layout of the LDS-DMA kernel: one 32-float K-tile per filter row = 8 pixels x 4 channels
        # (columns beyond kw are zero)
        if kw > 8:
            raise _lib.FgnHipError('pack_conv: a 4-channel (image) conv needs kw <= 8')
        w = weight.new_zeros(cout_pad, kh, 8, 4)
        w[:cout, :, :kw, :] = weight.permute(0, 2, 3, 1)
        w = w.reshape(cout_pad, kh * 32)
    else:
        k = kh * kw * cin
        k_pad = (k + 31) // 32 * 32
        w = weight.new_zeros(cout_pad, k_pad)
        w[:cout, :k] = weight.permute(0, 2, 3, 1).reshape(cout, k)
    scale = shift = None
    if bn is not None:
        scale = (bn['weight'].float() / torch.sqrt(bn['running_var'].float() + eps))
        shift = bn['bias'].float() - bn['running_mean'].float() * scale
        if bias is not None:
            shift = shift + bias.float() * scale
    elif bias is not None:
        shift = bias.detach().float().clone()
    pw = kh == 1 and kw == 1 and stride == 1 and pad == 0
    w3 = pack_x3(w) if (pw and _x3_ok(cin, cout)) else None
    wh = pack_h2(w) if ((pw and _h2_ok(cin, cout)) or (not pw and cin != 4 and _h2_conv_ok(cin, cout, kh, kw))) else None
    return ConvLayer(w.contiguous(), None if scale is None else scale.contiguous(),
                     None if shift is None else shift.contiguous(), cin, cout, cout_pad, kh, kw,
                     stride, pad, relu, w3, wh)


def conv2d(x: torch.Tensor, layer: ConvLayer, residual: Optional[torch.Tensor] = None,
           in_scale: Optional[torch.Tensor] = None, n_img_dev: Optional[torch.Tensor] = None,
           n_img: Optional[int] = None, a_img_div: int = 1, out: Optional[torch.Tensor] = None,
           tile_hint: int = 0) -> torch.Tensor:
    """x [n_in, H, W, Cin] -> y [n_img, Ho, Wo, Cout]; n_img defaults to n_in * a_img_div."""
    _chk(x, 'x')
    n_in, H, W, cin = x.shape
    if cin != layer.cin:
        raise _lib.FgnHipError(f'conv2d: Cin {cin} != layer Cin {layer.cin}')
    if n_img is None:
        n_img = n_in * a_img_div
    if n_img > n_in * a_img_div:
        raise _lib.FgnHipError('conv2d: n_img exceeds the input batch')
    ho = (H + 2 * layer.pad - layer.kh) // layer.stride + 1
    wo = (W + 2 * layer.pad - layer.kw) // layer.stride + 1
    if out is None:
        out = torch.empty((n_img, ho, wo, layer.cout), device=x.device, dtype=torch.float32)
    else:
        _chk(out, 'out')
        if tuple(out.shape) != (n_img, ho, wo, layer.cout):
            raise _lib.FgnHipError('conv2d: bad out shape')
    if residual is not None:
        _chk(residual, 'residual')
        if residual.shape != out.shape:
            raise _lib.FgnHipError('conv2d: residual shape mismatch')
    if in_scale is not None:
        _chk(in_scale, 'in_scale')
        if tuple(in_scale.shape) != (n_img, cin):
            raise _lib.FgnHipError(f'conv2d: in_scale must be [{n_img},{cin}], got {tuple(in_scale.shape)}')
    if n_img_dev is not None:
        _chk(n_img_dev, 'n_img_dev', torch.int32)
    prof = PROFILE
    L = _lib.load()
    if prof is not None:
        e0, e1 = prof.arm()
    pw = layer.kh == 1 and layer.kw == 1 and layer.stride == 1 and layer.pad == 0
    if layer.wh is not None and not pw and in_scale is None and a_img_div == 1 and tile_hint == 0 and residual is None and \
            n_img_dev is None and x.numel() * 4 < 0x7fffff00 and out.numel() < (1 << 31) and \
            L.fgn_h2_row_tile(n_img * ho * wo, layer.cout, layer.kh * layer.kw * cin, 0, 0) > 0:
        # 3x3 / strided convolution as an implicit GEMM on conv_pw_h2_kernel (one tensor)
        rc = L.fgn_conv2d_pair_h2_nhwc_f32(_ptr(x), n_img, H, W, None, 0, 1, 1, layer.wh.data_ptr(), _ptr(out), None,
                                           _ptr(layer.scale), _ptr(layer.shift), cin, layer.cout, layer.cout_pad, layer.kh,
                                           layer.kw, layer.stride, layer.pad, int(layer.relu), _stream())
        _lib.check(rc, 'fgn_conv2d_pair_h2_nhwc_f32')
        if prof is not None:
            k = layer.kh * layer.kw * cin
            flop = 2.0 * ho * wo * layer.cout * k
            prof.append(dict(kind='conv', kernel=h2_kernel(n_img * ho * wo, layer.cout, k, im2col=True), math='h2', e0=e0, e1=e1,
                             flop_direct=flop, flop_issued=flop, n_img=n_img, n_img_dev=None, gemm=(1, ho * wo, layer.cout, k),
                             residual=False, shape=(n_img, H, W, cin, layer.cout, layer.kh, layer.stride)))
        return out
    route = 'f32'
    if pw and in_scale is None and a_img_div == 1 and tile_hint == 0 and x.numel() * 4 < 0x7fffff00 and out.numel() < (1 << 31):
        route = _gemm_route(L, layer.w3, layer.wh, n_img * ho * wo, layer.cout, cin)
    if route != 'f32':
        name = 'fgn_conv1x1_%snhwc_f32' % _ROUTE_INFIX[route]
        rc = getattr(L, name)(_ptr(x), (layer.wh if route == 'h2' else layer.w3).data_ptr(), _ptr(out), _ptr(layer.scale),
                              _ptr(layer.shift), _ptr(residual), _ptr(n_img_dev), n_img, H, W, cin, layer.cout, layer.cout_pad,
                              int(layer.relu), _stream())
        _lib.check(rc, name)
        if prof is not None:
            flop = 2.0 * ho * wo * layer.cout * cin
            prof.append(dict(kind='conv', kernel=_gemm_kernel(route, None, n_img * ho * wo, layer.cout, cin),
                             math=route, e0=e0, e1=e1, flop_direct=flop, flop_issued=flop,
                             n_img=n_img, n_img_dev=n_img_dev, gemm=(1, ho * wo, layer.cout, cin),
                             residual=residual is not None, shape=(n_img, H, W, cin, layer.cout, 1, 1)))
        return out
    ws_bytes = L.fgn_conv2d_workspace_bytes(n_img, H, W, cin, layer.cout, layer.kh, layer.kw, layer.stride,
                                            layer.pad, tile_hint)
    ws = torch.empty(ws_bytes, device=x.device, dtype=torch.uint8) if ws_bytes else None
    rc = L.fgn_conv2d_nhwc_f32(
        _ptr(x), _ptr(layer.w), _ptr(out), _ptr(layer.scale), _ptr(layer.shift), _ptr(residual),
        _ptr(in_scale), _ptr(n_img_dev), n_img, H, W, cin, layer.cout, layer.cout_pad, layer.kh, layer.kw,
        layer.stride, layer.pad, a_img_div, int(layer.relu), tile_hint, _ptr(ws), ws_bytes, _stream())
    _lib.check(rc, 'fgn_conv2d_nhwc_f32')
    if prof is not None:
        kid = L.fgn_conv2d_kernel_id(n_img, H, W, cin, layer.cout, layer.cout_pad, layer.kh, layer.kw, layer.stride,
                                     layer.pad, a_img_div, int(in_scale is not None), int(residual is not None),
                                     tile_hint)
        flop = 2.0 * ho * wo * layer.cout * layer.kh * layer.kw * (3 if cin == 4 else cin)
        prof.append(dict(kind='conv', kernel=kernel_name(kid), e0=e0, e1=e1, flop_direct=flop,
                         flop_issued=flop, n_img=n_img, n_img_dev=n_img_dev,
                         gemm=(1, ho * wo, layer.cout, layer.kh * layer.kw * cin),       # groups, rows per image, N, K
                         residual=residual is not None,
                         shape=(n_img, H, W, cin, layer.cout, layer.kh, layer.stride)))
    return out


def pack_x3(w: torch.Tensor, mfma32: bool = False) -> torch.Tensor:
    """w [G, N, K] (or [N, K]) f32 -> the weight image of ``conv_pw_x3_kernel`` (csrc/conv_pw_x3.h): every value as the
    EXACT sum of three bf16 values (p1 = w with the low 16 bits cleared, p2 the same of w - p1, p3 = w - p1 - p2), laid
    out [G][K / 32][plane][Npad][32] bf16 with N padded to 128, the k order inside a K-tile that of the kernel's MFMA
    operand (chunk g = k 4g..4g+3, 16+4g..16+4g+3) and the four 16-byte chunks of a 64-byte row XOR-ed with
    tau[(n >> 2) & 3], tau = (0, 3, 2, 1) - tile by tile the LDS image the kernel's LDS-DMA writes, conflict-free for its
    ds_read_b128.  ``mfma32``: the image of the v_mfma_f32_32x32x16_bf16 instances of the experiments build (k in order,
    XOR with (n >> 2) & 3).  uint8 tensor on w's device."""
    w = w.detach().float()
    if w.dim() == 2:
        w = w[None]
    G, N, K = w.shape
    if K % 32:
        raise _lib.FgnHipError('pack_x3: K must be a multiple of 32')
    npad = (N + 127) // 128 * 128
    wp = w.new_zeros(G, npad, K)
    wp[:, :N] = w
    planes = []
    r = wp
    for _ in range(3):
        hi = (r.contiguous().view(torch.int32) & -65536).view(torch.float32)
        planes.append((hi.view(torch.int32) >> 16).to(torch.int16))
        r = r - hi                                     # exact: hi holds the leading bits of r
    pl = torch.stack(planes, 1)                        # [G, 3, npad, K] bf16 bit patterns
    sh16 = not mfma32
    if sh16:      # v_mfma_f32_16x16x32_bf16: lane group g reads the f32 chunks g and g + 4 of an activation row (conflict-free
        # in ds_read_b128's lane groups), so chunk g of a weight row holds k = 4g..4g+3, 16+4g..16+4g+3 of the K-tile
        korder = torch.tensor([4 * g + j if j < 4 else 16 + 4 * g + j - 4 for g in range(4) for j in range(8)], device=w.device)
        pl = pl.view(G, 3, npad, K // 32, 32)[..., korder]
    pl = pl.reshape(G, 3, npad, K // 32, 4, 8)         # K -> (K-tile, chunk, 8)
    n = torch.arange(npad, device=w.device)
    swz = (n >> 2) & 3
    if sh16:
        swz = torch.tensor([0, 3, 2, 1], device=w.device)[swz]
    src = torch.arange(4, device=w.device)[None, :] ^ swz[:, None]                       # physical chunk c holds logical c ^ swz
    pl = torch.gather(pl, 4, src[None, None, :, None, :, None].expand(G, 3, npad, K // 32, 4, 8))
    img = pl.permute(0, 3, 1, 2, 4, 5).contiguous()    # [G, KT, 3, npad, 4, 8]
    return img.view(torch.uint8).reshape(-1)


def gemm_x3(x: torch.Tensor, image: torch.Tensor, cout: int, shift: Optional[torch.Tensor] = None,
            residual: Optional[torch.Tensor] = None, relu: bool = False, groups: int = 1, grp_valid: Optional[int] = None,
            bm: int = 0, nterms: int = 6, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [rows, K] (grouped: [groups, grp_rows, K]) times the ``pack_x3`` image -> [rows, cout] on conv_pw_x3_kernel."""
    _chk(x, 'x')
    K = x.shape[-1]
    rows = x.numel() // K
    grp_rows = rows // groups
    npad = (cout + 127) // 128 * 128
    L = _lib.load()
    if image.numel() != L.fgn_x3_image_bytes(K, npad, groups):
        raise _lib.FgnHipError('gemm_x3: image size does not match K / cout / groups')
    if out is None:
        out = torch.empty(tuple(x.shape[:-1]) + (cout,), device=x.device, dtype=torch.float32)
    rc = L.fgn_gemm_x3_f32(_ptr(x), image.data_ptr(), _ptr(out), _ptr(shift), _ptr(residual), rows, K, cout, npad, int(relu),
                           grp_rows, grp_rows if grp_valid is None else grp_valid, groups, bm, nterms, _stream())
    _lib.check(rc, 'fgn_gemm_x3_f32')
    return out


def pack_h2(w: torch.Tensor) -> torch.Tensor:
    """w [G, N, K] (or [N, K]) f32 -> the weight image of ``conv_pw_h2_kernel`` (csrc/conv_pw_h2.h): every output column n of
    a group scaled by the power of two that puts its largest |w| into [2^14, 2^15) (an all-zero column: 1), then every value
    as two f16 planes, hi = f16(w s) and lo = f16(w s - hi) (round to nearest; hi + lo = w s to within 2^-23 |w s|: one f32 ulp at worst), laid
    out [G][K / 32][plane][Npad][32] f16 with ``pack_x3``'s k order and chunk swizzle, followed by the inverse scales
    [G][Npad] f32.  uint8 tensor on w's device."""
    w = w.detach().float()
    if w.dim() == 2:
        w = w[None]
    G, N, K = w.shape
    if K % 32:
        raise _lib.FgnHipError('pack_h2: K must be a multiple of 32')
    npad = (N + 127) // 128 * 128
    wp = w.new_zeros(G, npad, K)
    wp[:, :N] = w
    amax = wp.abs().amax(dim=2)                                              # [G, npad]
    e = torch.floor(torch.log2(torch.where(amax > 0, amax, torch.ones_like(amax)).double()))
    e = torch.where((amax > 0) & torch.isfinite(amax), e, torch.full_like(e, 14.0)).clamp_(-100.0, 100.0)
    scale = torch.pow(torch.tensor(2.0, dtype=torch.float64, device=w.device), 14.0 - e).float()
    inv = torch.pow(torch.tensor(2.0, dtype=torch.float64, device=w.device), e - 14.0).float()
    ws = wp * scale[:, :, None]                                              # exact (power of two)
    hi = ws.to(torch.float16)
    lo = (ws - hi.float()).to(torch.float16)
    pl = torch.stack((hi, lo), 1).view(torch.int16)                          # [G, 2, npad, K] f16 bit patterns
    korder = torch.tensor([4 * g + j if j < 4 else 16 + 4 * g + j - 4 for g in range(4) for j in range(8)], device=w.device)
    pl = pl.view(G, 2, npad, K // 32, 32)[..., korder]
    pl = pl.reshape(G, 2, npad, K // 32, 4, 8)                               # K -> (K-tile, chunk, 8)
    n = torch.arange(npad, device=w.device)
    swz = torch.tensor([0, 3, 2, 1], device=w.device)[(n >> 2) & 3]
    src = torch.arange(4, device=w.device)[None, :] ^ swz[:, None]           # physical chunk c holds logical c ^ swz
    pl = torch.gather(pl, 4, src[None, None, :, None, :, None].expand(G, 2, npad, K // 32, 4, 8))
    img = pl.permute(0, 3, 1, 2, 4, 5).contiguous()                          # [G, KT, 2, npad, 4, 8]
    return torch.cat((img.view(torch.uint8).reshape(-1), inv.contiguous().view(torch.uint8).reshape(-1)))


def gemm_h2(x: torch.Tensor, image: torch.Tensor, cout: int, shift: Optional[torch.Tensor] = None,
            residual: Optional[torch.Tensor] = None, relu: bool = False, groups: int = 1, grp_valid: Optional[int] = None,
            bm: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [rows, K] (grouped: [groups, grp_rows, K]) times the ``pack_h2`` image -> [rows, cout] on conv_pw_h2_kernel.
    bm: 0 = the library's choice, 64 / 128 / 264 = that tile on one K-group, 1064 = 64 rows on two K-groups."""
    _chk(x, 'x')
    K = x.shape[-1]
    rows = x.numel() // K
    grp_rows = rows // groups
    npad = (cout + 127) // 128 * 128
    L = _lib.load()
    if image.numel() != L.fgn_h2_image_bytes(K, npad, groups):
        raise _lib.FgnHipError('gemm_h2: image size does not match K / cout / groups')
    if out is None:
        out = torch.empty(tuple(x.shape[:-1]) + (cout,), device=x.device, dtype=torch.float32)
    rc = L.fgn_gemm_h2_f32(_ptr(x), image.data_ptr(), _ptr(out), _ptr(shift), _ptr(residual), rows, K, cout, npad, int(relu),
                           grp_rows, grp_rows if grp_valid is None else grp_valid, groups, bm, _stream())
    _lib.check(rc, 'fgn_gemm_h2_f32')
    return out


@dataclass
class DualConvLayer:
    """Two 1x1 / stride 1 convolutions with their eval-mode BatchNorms, packed for ONE K loop (``conv1x1_dual``):
    w [cout_pad, cin1 + cin2] with the two BN scales folded into its rows (fp64 fold, one rounding), shift = sum of the
    two BN shifts."""
    w: torch.Tensor
    shift: torch.Tensor
    cin1: int
    cin2: int
    cout: int
    cout_pad: int
    relu: bool
    w3: Optional[torch.Tensor] = None
    wh: Optional[torch.Tensor] = None

    def to(self, device):
        self.w, self.shift = self.w.to(device), self.shift.to(device)
        self.w3 = None if self.w3 is None else self.w3.to(device)
        self.wh = None if self.wh is None else self.wh.to(device)
        return self


def pack_conv_dual(w1: torch.Tensor, bn1: dict, w2: torch.Tensor, bn2: dict, relu: bool = True, eps: float = 1e-5) -> DualConvLayer:
    """w1 [Cout,Cin1,1,1] + bn1 (a bottleneck's conv3 / bn3), w2 [Cout,Cin2,1,1] + bn2 (its shortcut conv / bn)."""
    cout, cin1 = w1.shape[:2]
    cin2 = w2.shape[1]
    if tuple(w1.shape[2:]) != (1, 1) or tuple(w2.shape[2:]) != (1, 1) or w2.shape[0] != cout or cin1 % 32 or cin2 % 32 or cout % 4:
        raise _lib.FgnHipError('pack_conv_dual: two 1x1 kernels with one Cout, Cin1 / Cin2 multiples of 32, Cout % 4 == 0')
    rows, shift = [], 0.0
    for w, bn in ((w1, bn1), (w2, bn2)):
        sc = bn['weight'].double() / torch.sqrt(bn['running_var'].double() + eps)
        shift = shift + (bn['bias'].double() - bn['running_mean'].double() * sc)
        rows.append(w.detach().double().reshape(cout, -1) * sc[:, None])
    cout_pad = (cout + 127) // 128 * 128
    wp = torch.zeros(cout_pad, cin1 + cin2, dtype=torch.float32)
    wp[:cout] = torch.cat(rows, 1).float()
    return DualConvLayer(wp.contiguous(), shift.float().contiguous(), cin1, cin2, cout, cout_pad, relu,
                         pack_x3(wp) if _x3_ok(cin1 + cin2, cout) else None, pack_h2(wp) if _h2_ok(cin1 + cin2, cout) else None)


def strided_rows(shapes, stride: int, device) -> torch.Tensor:
    """Row table of a 1x1 / stride ``stride`` convolution over NHWC tensors that lie one behind the other in one buffer
    (``shapes`` = [(n, H, W), ...]): output row m (images, then output rows, then output columns, tensor after tensor) ->
    the input row it reads.  int32 on ``device``; for ``conv1x1_dual(..., x2_rows=)``."""
    out, base = [], 0
    for n, H, W in shapes:
        ho, wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        img = torch.arange(n, dtype=torch.int64)[:, None, None] * (H * W)
        oy = torch.arange(ho, dtype=torch.int64)[None, :, None] * (stride * W)
        ox = torch.arange(wo, dtype=torch.int64)[None, None, :] * stride
        out.append((base + img + oy + ox).reshape(-1))
        base += n * H * W
    return torch.cat(out).to(torch.int32).to(device)


def conv1x1_dual(x1: torch.Tensor, x2: torch.Tensor, layer: DualConvLayer, out: Optional[torch.Tensor] = None,
                 x2_rows: Optional[torch.Tensor] = None, bm: int = 0) -> torch.Tensor:
    """x1 [..., Cin1] -> relu?(x1 W1^T + x2' W2^T + shift) [..., Cout], x2' = x2 over the same leading dims (rows), or -
    with ``x2_rows`` (int32 [rows], ``strided_rows``) - row x2_rows[m] of x2 [..., Cin2] for output row m.
    bm != 0 (tests, tools): conv_pw_h2_kernel_dual with that tile code forced (``gemm_h2``)."""
    _chk(x1, 'x1')
    _chk(x2, 'x2')
    rows = x1.numel() // layer.cin1
    if x1.shape[-1] != layer.cin1 or x2.shape[-1] != layer.cin2 or (x2_rows is None and x1.shape[:-1] != x2.shape[:-1]):
        raise _lib.FgnHipError('conv1x1_dual: operand shapes inconsistent with the layer')
    x2_total = x2.numel() // layer.cin2
    if x2_rows is not None:
        _chk(x2_rows, 'x2_rows', torch.int32)
        if x2_rows.numel() != rows:
            raise _lib.FgnHipError('conv1x1_dual: x2_rows must hold one input row per output row')
    shape = tuple(x1.shape[:-1]) + (layer.cout,)
    if out is None:
        out = torch.empty(shape, device=x1.device, dtype=torch.float32)
    else:
        _chk(out, 'out')
        if tuple(out.shape) != shape:
            raise _lib.FgnHipError('conv1x1_dual: bad out shape')
    prof = PROFILE
    L = _lib.load()
    if prof is not None:
        e0, e1 = prof.arm()
    k = layer.cin1 + layer.cin2
    route = 'f32'
    if max(x1.numel(), x2.numel()) * 4 < 0x7fffff00:
        route = _gemm_route(L, layer.w3, layer.wh, rows, layer.cout, k)
    if bm != 0:
        if layer.wh is None or max(x1.numel(), x2.numel()) * 4 >= 0x7fffff00:
            raise _lib.FgnHipError('conv1x1_dual: a forced tile code needs a layer packed for conv_pw_h2_kernel')
        route = 'h2'
        rc = L.fgn_conv1x1_dual_h2_bm_nhwc_f32(_ptr(x1), _ptr(x2), _ptr(x2_rows), x2_total, layer.wh.data_ptr(), _ptr(out),
                                               _ptr(layer.shift), rows, layer.cin1, layer.cin2, layer.cout, layer.cout_pad,
                                               int(layer.relu), bm, _stream())
    else:
        w = {'h2': layer.wh, 'x3': layer.w3, 'f32': layer.w}[route]
        rc = getattr(L, 'fgn_conv1x1_dual_%snhwc_f32' % _ROUTE_INFIX[route])(
            _ptr(x1), _ptr(x2), _ptr(x2_rows), x2_total, w.data_ptr(), _ptr(out), _ptr(layer.shift), rows, layer.cin1, layer.cin2,
            layer.cout, layer.cout_pad, int(layer.relu), _stream())
    _lib.check(rc, 'fgn_conv1x1_dual_nhwc_f32')
    if prof is not None:
        flop = 2.0 * rows * layer.cout * k
        kernel = h2_dual_kernel(rows, layer.cout, k, bm) if route == 'h2' else \
            _gemm_kernel(route, 'conv_pw_persist_kernel', rows, layer.cout, k)
        prof.append(dict(kind='conv', kernel=kernel,
                         math=route, e0=e0, e1=e1, flop_direct=flop, flop_issued=flop,
                         n_img=1, n_img_dev=None, gemm=(1, rows, layer.cout, k), residual=False,
                         shape=(1, rows, 1, k, layer.cout, 1, 1)))
    return out


def conv2d_pair(x0: torch.Tensor, x1: torch.Tensor, layer: ConvLayer, out0: Optional[torch.Tensor] = None,
                out1: Optional[torch.Tensor] = None, bm: int = 0):
    """The same convolution (weights, folded BN, ReLU) on two NHWC tensors of different geometry in ONE launch - the
    query map and the support maps of a backbone layer that strides over the spatial structure (3x3 / stride 2, the
    1x1 / stride 2 shortcut, the stem).  Per tensor the arithmetic of ``conv2d`` without split-K.  -> (y0, y1).
    bm != 0 (tests, tools): the implicit GEMM on conv_pw_h2_kernel with that tile code forced (``gemm_h2``)."""
    _chk(x0, 'x0')
    _chk(x1, 'x1')
    if x0.shape[3] != layer.cin or x1.shape[3] != layer.cin:
        raise _lib.FgnHipError(f'conv2d_pair: Cin {x0.shape[3]} / {x1.shape[3]} != layer Cin {layer.cin}')
    outs = []
    for x, out in ((x0, out0), (x1, out1)):
        n, H, W, _ = x.shape
        ho = (H + 2 * layer.pad - layer.kh) // layer.stride + 1
        wo = (W + 2 * layer.pad - layer.kw) // layer.stride + 1
        if out is None:
            out = torch.empty((n, ho, wo, layer.cout), device=x.device, dtype=torch.float32)
        else:
            _chk(out, 'out')
            if tuple(out.shape) != (n, ho, wo, layer.cout):
                raise _lib.FgnHipError('conv2d_pair: bad out shape')
        outs.append(out)
    prof = PROFILE
    L = _lib.load()
    if prof is not None:
        e0, e1 = prof.arm()
    rows = sum(o.shape[0] * o.shape[1] * o.shape[2] for o in outs)
    k = layer.kh * layer.kw * layer.cin
    span = abs(x0.data_ptr() - x1.data_ptr()) + max(x0.numel(), x1.numel()) * 4
    if bm != 0:
        if layer.wh is None or layer.cin == 4 or span >= 0x7fffff00 or rows * layer.cout >= (1 << 31):
            raise _lib.FgnHipError('conv2d_pair: a forced tile code needs a layer packed for conv_pw_h2_kernel')
        rc = L.fgn_conv2d_pair_h2_bm_nhwc_f32(_ptr(x0), x0.shape[0], x0.shape[1], x0.shape[2], _ptr(x1), x1.shape[0], x1.shape[1],
                                              x1.shape[2], layer.wh.data_ptr(), _ptr(outs[0]), _ptr(outs[1]), _ptr(layer.scale),
                                              _ptr(layer.shift), layer.cin, layer.cout, layer.cout_pad, layer.kh, layer.kw,
                                              layer.stride, layer.pad, int(layer.relu), bm, _stream())
        _lib.check(rc, 'fgn_conv2d_pair_h2_bm_nhwc_f32')
        return outs[0], outs[1]
    if layer.wh is not None and layer.cin != 4 and span < 0x7fffff00 and rows * layer.cout < (1 << 31) and \
            L.fgn_h2_row_tile(rows, layer.cout, k, 0, 0) > 0:
        # the implicit GEMM of both tensors on conv_pw_h2_kernel
        rc = L.fgn_conv2d_pair_h2_nhwc_f32(_ptr(x0), x0.shape[0], x0.shape[1], x0.shape[2], _ptr(x1), x1.shape[0], x1.shape[1],
                                           x1.shape[2], layer.wh.data_ptr(), _ptr(outs[0]), _ptr(outs[1]), _ptr(layer.scale),
                                           _ptr(layer.shift), layer.cin, layer.cout, layer.cout_pad, layer.kh, layer.kw,
                                           layer.stride, layer.pad, int(layer.relu), _stream())
        _lib.check(rc, 'fgn_conv2d_pair_h2_nhwc_f32')
        if prof is not None:
            flop = 2.0 * layer.cout * k * rows
            prof.append(dict(kind='conv', kernel=h2_kernel(rows, layer.cout, k, im2col=True), math='h2', e0=e0, e1=e1,
                             flop_direct=flop, flop_issued=flop, n_img=1, n_img_dev=None, gemm=(1, rows, layer.cout, k),
                             shape=(x0.shape[0] + x1.shape[0], x0.shape[1], x0.shape[2], layer.cin, layer.cout, layer.kh,
                                    layer.stride)))
        return outs[0], outs[1]
    rc = L.fgn_conv2d_pair_nhwc_f32(_ptr(x0), _ptr(outs[0]), x0.shape[0], x0.shape[1], x0.shape[2],
                                    _ptr(x1), _ptr(outs[1]), x1.shape[0], x1.shape[1], x1.shape[2],
                                    _ptr(layer.w), _ptr(layer.scale), _ptr(layer.shift), layer.cin, layer.cout,
                                    layer.cout_pad, layer.kh, layer.kw, layer.stride, layer.pad, int(layer.relu), _stream())
    _lib.check(rc, 'fgn_conv2d_pair_nhwc_f32')
    if prof is not None:
        per_px = 2.0 * layer.cout * layer.kh * layer.kw * (3 if layer.cin == 4 else layer.cin)
        flop = per_px * sum(o.shape[0] * o.shape[1] * o.shape[2] for o in outs)
        prof.append(dict(kind='conv', kernel='conv_igemm_dma_pair_kernel<64, 64, 32, 32, 2, 4, %d>' % (2 if layer.cin == 4 else 0),
                         e0=e0, e1=e1, flop_direct=flop, flop_issued=flop, n_img=1, n_img_dev=None,
                         gemm=(1, sum(o.shape[0] * o.shape[1] * o.shape[2] for o in outs), layer.cout,
                               layer.kh * layer.kw * (3 if layer.cin == 4 else layer.cin)),
                         shape=(x0.shape[0] + x1.shape[0], x0.shape[1], x0.shape[2], layer.cin, layer.cout, layer.kh,
                                layer.stride)))
    return outs[0], outs[1]


# --------------------------------------------------------------------------------------
# Winograd F(2x2,3x3) form of 3x3 / stride 1 / pad 1 convolutions
# --------------------------------------------------------------------------------------
@dataclass
class WinogradLayer:
    """U [m_in^2, cout_pad, Cin] = G w G^T with the per-channel epilogue scale folded in; shift [Cout].
    ``m`` = output tile edge: 4 = F(4x4,3x3), 36 tile positions; 2 = F(2x2,3x3), 16 positions."""
    u: torch.Tensor
    shift: Optional[torch.Tensor]
    cin: int
    cout: int
    cout_pad: int
    relu: bool
    m: int = 2
    u3: Optional[torch.Tensor] = None      # bf16-plane image of u (pack_x3), or None
    uh: Optional[torch.Tensor] = None      # f16-plane image of u (pack_h2), or None

    @property
    def groups(self) -> int:
        return (self.m + 2) ** 2

    def to(self, device):
        self.u = self.u.to(device)
        self.shift = None if self.shift is None else self.shift.to(device)
        self.u3 = None if self.u3 is None else self.u3.to(device)
        self.uh = None if self.uh is None else self.uh.to(device)
        return self


_WG_G = {
    2: torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64),
    # Cook-Toom, points {0, 1, -1, 1/2, -2, inf} (csrc/winograd.hip holds the matching B^T / A^T)
    4: torch.tensor([[1.0, 0.0, 0.0], [1 / 3, 1 / 3, 1 / 3], [-1 / 3, 1 / 3, -1 / 3], [-16 / 15, -8 / 15, -4 / 15],
                     [1 / 15, -2 / 15, 4 / 15], [0.0, 0.0, 1.0]], dtype=torch.float64),
}
WINOGRAD_M = 4       # default output tile edge
_WG_MIN_CIN = int(os.environ.get('FGN_WG_MIN_CIN', '128'))    # F(4x4) from this many input channels (A/B knob: see winograd_pays)


def pack_winograd(weight: torch.Tensor, bias: Optional[torch.Tensor] = None, bn: Optional[dict] = None,
                  relu: bool = False, eps: float = 1e-5, m: Optional[int] = None) -> WinogradLayer:
    """weight [Cout,Cin,3,3] -> WinogradLayer (transform in fp64, stored fp32)."""
    m = WINOGRAD_M if m is None else m
    cout, cin, kh, kw = weight.shape
    if (kh, kw) != (3, 3) or cin % 32 != 0 or cout % 4 != 0 or m not in _WG_G:
        raise _lib.FgnHipError('pack_winograd: needs a 3x3 kernel, Cin % 32 == 0, Cout % 4 == 0, m in (2, 4)')
    w = weight.detach().double()
    scale = shift = None
    if bn is not None:
        scale = bn['weight'].double() / torch.sqrt(bn['running_var'].double() + eps)
        shift = bn['bias'].double() - bn['running_mean'].double() * scale
        if bias is not None:
            shift = shift + bias.double() * scale
        w = w * scale[:, None, None, None]
    elif bias is not None:
        shift = bias.detach().double()
    G = _WG_G[m].to(w.device)
    u = torch.einsum('ai,ocij,bj->aboc', G, w, G)                            # [m+2,m+2,Cout,Cin]
    cout_pad = (cout + 127) // 128 * 128
    up = torch.zeros((m + 2) ** 2, cout_pad, cin, dtype=torch.float32, device=w.device)
    up[:, :cout] = u.reshape((m + 2) ** 2, cout, cin).float()
    return WinogradLayer(up.contiguous(), None if shift is None else shift.float().contiguous(), cin, cout,
                         cout_pad, relu, m, pack_x3(up) if _x3_ok(cin, cout) else None, pack_h2(up) if _h2_ok(cin, cout) else None)


_WG_G_DEV: dict = {}


def repack_conv_(layer: ConvLayer, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> ConvLayer:
    """``pack_conv`` of updated weights INTO an existing packed layer (no BatchNorm fold, Cin != 4): one strided copy -
    what a training step needs after its optimizer update.  The padding rows / columns keep the zeros of the first pack."""
    cout, cin, kh, kw = weight.shape
    if (cout, cin, kh, kw) != (layer.cout, layer.cin, layer.kh, layer.kw) or cin == 4 or layer.scale is not None:
        raise _lib.FgnHipError('repack_conv_: layer and weight do not match (or the layer folds a BatchNorm)')
    k = kh * kw * cin
    if layer.w.shape[1] == k:                      # rows are exactly K long: one strided copy
        layer.w[:cout].view(cout, kh, kw, cin).copy_(weight.detach().permute(0, 2, 3, 1))
    else:                                          # K padded to a multiple of 32: through a contiguous temporary
        layer.w[:cout, :k].copy_(weight.detach().permute(0, 2, 3, 1).reshape(cout, k))
    if bias is not None:
        layer.shift.copy_(bias.detach())
    if layer.w3 is not None:
        layer.w3.copy_(pack_x3(layer.w))
    if layer.wh is not None:
        layer.wh.copy_(pack_h2(layer.w))
    return layer


def repack_winograd_(layer: WinogradLayer, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> WinogradLayer:
    """``pack_winograd`` of updated weights INTO an existing layer: one kernel (``fgn_winograd_pack_weights_f32``, fp64
    arithmetic on the device, one rounding - the host transform's arithmetic) instead of ~40 torch kernels."""
    cout, cin, kh, kw = weight.shape
    if (cout, cin, kh, kw) != (layer.cout, layer.cin, 3, 3):
        raise _lib.FgnHipError('repack_winograd_: layer and weight do not match')
    w = weight.detach()
    _chk(w, 'weight')
    key = (layer.m, w.device)
    G = _WG_G_DEV.get(key)
    if G is None:
        G = _WG_G_DEV[key] = _WG_G[layer.m].to(w.device).contiguous()
    rc = _lib.load().fgn_winograd_pack_weights_f32(_ptr(w), _ptr(G), _ptr(layer.u), cout, cin, layer.cout_pad, layer.m,
                                                   _stream())
    _lib.check(rc, 'fgn_winograd_pack_weights_f32')
    if bias is not None:
        layer.shift.copy_(bias.detach())
    if layer.u3 is not None:
        layer.u3.copy_(pack_x3(layer.u))
    if layer.uh is not None:
        layer.uh.copy_(pack_h2(layer.u))
    return layer


def _wg_tiles(H: int, W: int, m: int) -> int:
    return ((H + m - 1) // m) * ((W + m - 1) // m)


def winograd_fits(n_img: int, H: int, W: int, cin: int, cout: int, m: Optional[int] = None) -> bool:
    """The grouped GEMM addresses V / Mo through 32-bit buffer offsets: [groups * t_pad, C] must stay below 2 GiB."""
    m = WINOGRAD_M if m is None else m
    t_pad = (n_img * _wg_tiles(H, W, m) + 63) // 64 * 64
    rows = (m + 2) ** 2 * t_pad
    return rows * cin * 4 < 0x7fffff00 and rows * cout < (1 << 31)


def winograd_pays(n_img: int, H: int, W: int, cin: int, cout: int, m: Optional[int] = None) -> bool:
    """Measured on MI355X (tools/wg_bench.py, direct -> F(2x2) -> F(4x4)): AG-RPN conv 2.23 -> 0.95 -> 0.57 ms,
    shared_head 3x3 on 300 RoIs 0.65 -> 0.43 -> 0.29 ms, layer1 (64 channels, 200x334) 65 -> 70 -> 57 us; the
    9-RoI support head (441 pixels) loses to the launch costs of the three kernels.  Both forms need about a thousand
    output pixels and 128 input channels.  (Alone, F(4x4) wins at 64 channels too - layer1: 57 us against 65 for the direct
    form - but its three launches move 5.5x the bytes, and in the pipelined step, beside the other episode's GEMMs, the
    direct form wins: round 5, same box, three interleaved pairs 203.2-204.0 -> 204.4-204.8 img/s.)"""
    m = WINOGRAD_M if m is None else m
    return cin >= (_WG_MIN_CIN if m == 4 else 128) and n_img * H * W >= 1024 and winograd_fits(n_img, H, W, cin, cout, m)


def _winograd_gemm(L, layer: WinogradLayer, V, Mo, n_img_dev, n_img: int, tiles: int, t_pad: int, st) -> str:
    """The grouped GEMM Mo = V U^T of a Winograd convolution (n_img x tiles valid rows per group).  -> its route."""
    route = _gemm_route(L, layer.u3, layer.uh, layer.groups * t_pad, layer.cout, layer.cin, t_pad, n_img * tiles)
    name = 'fgn_winograd_gemm_%sf32' % _ROUTE_INFIX[route]
    u = {'h2': layer.uh, 'x3': layer.u3, 'f32': layer.u}[route]
    _lib.check(getattr(L, name)(_ptr(V), u.data_ptr(), _ptr(Mo), _ptr(n_img_dev), n_img, tiles, t_pad, layer.cin, layer.cout,
                                layer.cout_pad, layer.groups, st), name)
    return route


def _winograd_records(prof, ev, L, layer: WinogradLayer, route: str, t_pad: int, valid: int, tiles: int, pixels: int,
                      bits=(64, 64), **common) -> None:
    """The three PROFILE records of a Winograd convolution (ev: the event pairs of input transform, GEMM, output transform).
    ``valid`` tiles are computed per group; a record's FLOPs are per image of ``tiles`` tiles and ``pixels`` pixels.
    ``bits``: the index width (``winograd4_index_bits``) of the input / output transform launch: 32 = the narrow instance."""
    G, cin, cout = layer.groups, layer.cin, layer.cout
    kin, kout = 'wg_input_kernel', 'wg_output_kernel'
    if layer.m == 4:     # the template instances of the F(4x4) transforms (csrc/winograd.hip): <vector width, eager>
        vi, vo = L.fgn_winograd4_variant(valid, cin, 0), L.fgn_winograd4_variant(valid, cout, 1)
        kin = 'wg4_input_kernel<%d, %s>' % (vi // 10, 'true' if vi % 10 else 'false')
        kout = 'wg4_output_kernel<%d>' % (vo // 10)
        if bits[0] == 32:
            kin = 'wg4_input_narrow_kernel<%d>' % (vi // 10)
        if bits[1] == 32:
            kout = 'wg4_output_narrow_kernel<%d>' % (vo // 10)
    prof.append(dict(kind='wg_in', kernel=kin, e0=ev[0][0], e1=ev[0][1], flop_direct=0.0, flop_issued=0.0, **common))
    # direct-convolution FLOPs of the layer (what the reference's formulation executes) are booked on the GEMM record; the
    # MFMA work issued is (m+2)^2 products per m x m output tile instead of 9 m^2.  The GEMM: point-wise over [G * t_pad] rows
    gid = L.fgn_conv2d_kernel_id(G * t_pad, 1, 1, cin, cout, layer.cout_pad, 1, 1, 1, 0, 1, 0, 0, 4)   # 64x64 tile
    prof.append(dict(kind='wg_gemm', kernel=_gemm_kernel(route, kernel_name(gid), G * t_pad, cout, cin, t_pad, valid),
                     math=route, e0=ev[1][0], e1=ev[1][1], flop_direct=2.0 * pixels * cout * 9 * cin,
                     flop_issued=2.0 * G * tiles * cout * cin, gemm=(G, tiles, cout, cin), **common))
    prof.append(dict(kind='wg_out', kernel=kout, e0=ev[2][0], e1=ev[2][1], flop_direct=0.0, flop_issued=0.0, **common))


def conv3x3_winograd(x: torch.Tensor, layer: WinogradLayer, in_scale: Optional[torch.Tensor] = None,
                     a_img_div: int = 1, n_img_dev: Optional[torch.Tensor] = None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [n_in,H,W,Cin] -> relu?(conv3x3(x[i // a_img_div] * in_scale[i]) + shift) [n_in*a_img_div,H,W,Cout].
    ``out``: a caller-owned result tensor (images past a device count keep their bytes)."""
    _chk(x, 'x')
    n_in, H, W, cin = x.shape
    if cin != layer.cin:
        raise _lib.FgnHipError(f'conv3x3_winograd: Cin {cin} != layer Cin {layer.cin}')
    n_img = n_in * a_img_div
    if in_scale is not None:
        _chk(in_scale, 'in_scale')
        if tuple(in_scale.shape) != (n_img, cin):
            raise _lib.FgnHipError('conv3x3_winograd: in_scale must be [n_img, Cin]')
    if n_img_dev is not None:
        _chk(n_img_dev, 'n_img_dev', torch.int32)
    tiles = _wg_tiles(H, W, layer.m)
    L = _lib.load()
    f_in, f_out = (L.fgn_winograd4_input_f32, L.fgn_winograd4_output_f32) if layer.m == 4 else \
        (L.fgn_winograd_input_f32, L.fgn_winograd_output_f32)
    G = layer.groups
    t_pad = L.fgn_winograd_t_pad(n_img * tiles)
    V = torch.empty((G, t_pad, cin), device=x.device, dtype=torch.float32)
    Mo = torch.empty((G, t_pad, layer.cout), device=x.device, dtype=torch.float32)
    if out is None:
        y = torch.empty((n_img, H, W, layer.cout), device=x.device, dtype=torch.float32)
    else:
        _chk(out, 'out')
        if tuple(out.shape) != (n_img, H, W, layer.cout):
            raise _lib.FgnHipError('conv3x3_winograd: bad out shape')
        y = out
    prof = PROFILE
    st = _stream()
    ev = [] if prof is not None else None
    if ev is not None:
        ev.append(prof.arm())
    _lib.check(f_in(_ptr(x), _ptr(in_scale), _ptr(V), _ptr(n_img_dev), n_img, a_img_div, H, W, cin, t_pad, st),
               'fgn_winograd_input_f32')
    if ev is not None:
        ev.append(prof.arm())
    route = _winograd_gemm(L, layer, V, Mo, n_img_dev, n_img, tiles, t_pad, st)
    if ev is not None:
        ev.append(prof.arm())
    _lib.check(f_out(_ptr(Mo), _ptr(y), _ptr(layer.shift), _ptr(n_img_dev), n_img, H, W, layer.cout, t_pad,
                     int(layer.relu), st), 'fgn_winograd_output_f32')
    if ev is not None:
        bits = (64, 64) if layer.m != 4 else (
            winograd4_index_bits(n_img, H, W, cin, t_pad, a_img_div=a_img_div, with_scale=in_scale is not None),
            winograd4_index_bits(n_img, H, W, layer.cout, t_pad, output=True))
        _winograd_records(prof, ev, L, layer, route, t_pad, n_img * tiles, tiles, H * W, bits=bits, n_img=n_img, n_img_dev=n_img_dev,
                          shape=(n_img, H, W, cin, layer.cout, 3, 1))
    return y


def winograd4_index_bits(n_img: int, H: int, W: int, C: int, t_pad: int, a_img_div: int = 1, second=None,
                         with_scale: bool = False, output: bool = False) -> int:
    """32 / 64: the index width the F(4x4) input (``output``: output) transform takes at these sizes (``second`` = (n, H, W)
    of a second tensor): the launchers' own rule.  Computed from the sizes; nothing is allocated."""
    n1, h1, w1 = second if second is not None else (0, 1, 1)
    return _lib.load().fgn_winograd4_index_bits(n_img, a_img_div, H, W, n1, h1, w1, C, t_pad, int(with_scale), int(output))


def winograd4_input(x: torch.Tensor, V: torch.Tensor, in_scale: Optional[torch.Tensor] = None, a_img_div: int = 1,
                    n_img_dev: Optional[torch.Tensor] = None, x1: Optional[torch.Tensor] = None, index_bits: int = 0,
                    vec: int = 0) -> None:
    """The F(4x4) input transform alone (tests, tools): x [n_in,H,W,C] (and ``x1`` behind it) -> V [36,t_pad,C] in place,
    with the kernel instance forced: index_bits 32 (narrow) / 64 (wide) / 0 (by the sizes); vec 1 / 2 / 4 channels per
    thread / 0 (the library's rule)."""
    _chk(x, 'x')
    _chk(V, 'V')
    n_in, H, W, C = x.shape
    n1, h1, w1 = (0, 1, 1) if x1 is None else tuple(x1.shape[:3])
    rc = _lib.load().fgn_winograd4_input_ix_f32(_ptr(x), _ptr(in_scale), _ptr(V), _ptr(n_img_dev), n_in * a_img_div, a_img_div,
                                                H, W, C, V.shape[1], _ptr(x1), n1, h1, w1, index_bits, vec, _stream())
    _lib.check(rc, 'fgn_winograd4_input_ix_f32')


def winograd4_output(Mo: torch.Tensor, y: torch.Tensor, shift: Optional[torch.Tensor] = None, relu: bool = False,
                     n_img_dev: Optional[torch.Tensor] = None, y1: Optional[torch.Tensor] = None, index_bits: int = 0,
                     vec: int = 0) -> None:
    """The F(4x4) output transform alone (tests, tools): Mo [36,t_pad,C] -> y [n,H,W,C] (and ``y1``) in place, with the
    kernel instance forced as for ``winograd4_input``."""
    _chk(Mo, 'Mo')
    _chk(y, 'y')
    n, H, W, C = y.shape
    n1, h1, w1 = (0, 1, 1) if y1 is None else tuple(y1.shape[:3])
    rc = _lib.load().fgn_winograd4_output_ix_f32(_ptr(Mo), _ptr(y), _ptr(shift), _ptr(n_img_dev), n, H, W, C, Mo.shape[1],
                                                 int(relu), _ptr(y1), n1, h1, w1, index_bits, vec, _stream())
    _lib.check(rc, 'fgn_winograd4_output_ix_f32')


def conv3x3_winograd_multi(xs, layer: WinogradLayer, outs) -> None:
    """The F(4x4) / F(2x2) convolution of SEVERAL inputs with one weight set through ONE grouped GEMM: every input
    [n_i, H_i, W_i, Cin] is transformed into its own tile range of a shared V, the GEMM runs over all tiles, every
    output ``outs[i]`` [n_i, H_i, W_i, Cout] (views of a caller-owned buffer) is transformed out of its range of Mo.
    (The transforms address tile t of position g at ((g * t_pad + t) * C): a tile offset is a pointer offset.)"""
    L = _lib.load()
    f_in, f_out = (L.fgn_winograd4_input_f32, L.fgn_winograd4_output_f32) if layer.m == 4 else \
        (L.fgn_winograd_input_f32, L.fgn_winograd_output_f32)
    cin, cout, G = layer.cin, layer.cout, layer.groups
    tiles = []
    for x, y in zip(xs, outs):
        _chk(x, 'x')
        _chk(y, 'out')
        if x.shape[-1] != cin or tuple(y.shape) != tuple(x.shape[:-1]) + (cout,):
            raise _lib.FgnHipError('conv3x3_winograd_multi: operand shapes inconsistent')
        tiles.append(x.shape[0] * _wg_tiles(x.shape[1], x.shape[2], layer.m))
    total = sum(tiles)
    t_pad = L.fgn_winograd_t_pad(total)
    if G * t_pad * max(cin, cout) * 4 >= 0x7fffff00:
        raise _lib.FgnHipError('conv3x3_winograd_multi: V / Mo exceed the 2 GiB descriptors')
    dev = xs[0].device
    V = torch.empty((G, t_pad, cin), device=dev, dtype=torch.float32)
    Mo = torch.empty((G, t_pad, cout), device=dev, dtype=torch.float32)
    st = _stream()
    pair = layer.m == 4 and len(xs) == 2          # one transform launch for both tensors
    prof = PROFILE if pair else None              # (the per-tensor form is not instrumented: tests / F(2x2) only)
    ev = []
    if prof is not None:
        ev.append(prof.arm())
    if pair:
        (n0, h0, w0, _), (n1, h1, w1, _) = xs[0].shape, xs[1].shape
        _lib.check(L.fgn_winograd4_input2_f32(_ptr(xs[0]), n0, h0, w0, _ptr(xs[1]), n1, h1, w1, _ptr(V), cin, t_pad, st),
                   'fgn_winograd4_input2_f32')
    else:
        off = 0
        for x, n_t in zip(xs, tiles):
            n, H, W, _ = x.shape
            _lib.check(f_in(_ptr(x), None, V.data_ptr() + off * cin * 4, None, n, 1, H, W, cin, t_pad, st),
                       'fgn_winograd_input_f32')
            off += n_t
    if prof is not None:
        ev.append(prof.arm())
    route = _winograd_gemm(L, layer, V, Mo, None, 1, total, t_pad, st)
    if prof is not None:
        ev.append(prof.arm())
    if pair:
        _lib.check(L.fgn_winograd4_output2_f32(_ptr(Mo), _ptr(layer.shift), _ptr(outs[0]), n0, h0, w0, _ptr(outs[1]), n1, h1,
                                               w1, cout, t_pad, int(layer.relu), st), 'fgn_winograd4_output2_f32')
    else:
        off = 0
        for y, n_t in zip(outs, tiles):
            n, H, W, _ = y.shape
            _lib.check(f_out(Mo.data_ptr() + off * cout * 4, _ptr(y), _ptr(layer.shift), None, n, H, W, cout, t_pad,
                             int(layer.relu), st), 'fgn_winograd_output_f32')
            off += n_t
    if prof is not None:
        pixels = sum(x.shape[0] * x.shape[1] * x.shape[2] for x in xs)
        bits = (winograd4_index_bits(n0, h0, w0, cin, t_pad, second=(n1, h1, w1)),
                winograd4_index_bits(n0, h0, w0, cout, t_pad, second=(n1, h1, w1), output=True))
        _winograd_records(prof, ev, L, layer, route, t_pad, total, total, pixels, bits=bits, n_img=1, n_img_dev=None,
                          shape=(len(xs), pixels, 1, cin, cout, 3, 1))


# --------------------------------------------------------------------------------------
# spatial ops
# --------------------------------------------------------------------------------------
def nchw3_to_nhwc4(x: torch.Tensor) -> torch.Tensor:
    _chk(x, 'x')
    n, c, h, w = x.shape
    if c != 3:
        raise _lib.FgnHipError('nchw3_to_nhwc4: expects 3 channels')
    y = torch.empty((n, h, w, 4), device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().fgn_nchw3_to_nhwc4_f32(_ptr(x), _ptr(y), n, h, w, _stream()),
               'fgn_nchw3_to_nhwc4_f32')
    return y


def input_lut(mean, std, scale: float = 255.0) -> np.ndarray:
    """The normalisation table of ``u8hwc3_to_nhwc4``: lut[c][v] = (float32(v) / scale - mean[c]) / std[c] in float32
    numpy arithmetic, exactly what the data loader computes per pixel (``ClutteredCharsFewShotISEG._norm``; bit-equal to
    torch's ``float().div(255).sub(mean).div(std)``).  [3,256] float32."""
    mean, std = np.asarray(mean, np.float32).reshape(3), np.asarray(std, np.float32).reshape(3)
    v = np.arange(256, dtype=np.uint8)[:, None]
    return np.ascontiguousarray(((v.astype(np.float32) / scale - mean) / std).T)


# pixels one pass of u8hwc3_to_nhwc4_kernel's grid-stride loop covers: U8_GRID_CAP workgroups x 256 lanes x 4 pixels
# (csrc/spatial.hip)
U8_PIXELS_PER_PASS = 256 * 8 * 256 * 4


def u8hwc3_to_nhwc4(x_u8: torch.Tensor, lut: torch.Tensor) -> torch.Tensor:
    """uint8 channels-last [n,H,W,3] -> NHWC4 fp32 [n,H,W,4], normalised through ``lut`` ([3,256] fp32 on the device,
    from ``input_lut``): the bytes ``nchw3_to_nhwc4`` gives for the host-normalised image.  ``x_u8`` may start at any
    byte (a sliced view)."""
    _chk(x_u8, 'x_u8', torch.uint8)
    _chk(lut, 'lut')
    if x_u8.dim() != 4 or x_u8.shape[3] != 3:
        raise _lib.FgnHipError('u8hwc3_to_nhwc4: expects [n,H,W,3]')
    if tuple(lut.shape) != (3, 256) or lut.device != x_u8.device:
        raise _lib.FgnHipError('u8hwc3_to_nhwc4: lut must be [3,256] on the device of x_u8')
    n, h, w, _ = x_u8.shape
    y = torch.empty((n, h, w, 4), device=x_u8.device, dtype=torch.float32)
    if y.numel() == 0:                  # (an empty tensor has no address to hand over)
        return y
    _lib.check(_lib.load().fgn_u8hwc3_to_nhwc4_f32(_ptr(x_u8), _ptr(lut), _ptr(y), n, h, w, _stream()),
               'fgn_u8hwc3_to_nhwc4_f32')
    return y


RESIZE_MAX_DIM = 16384       # csrc/spatial.hip; fewshot_ds.RESIZE_MAX_DIM: int32 arithmetic of the resize rule
AUG_REC_INTS = 16            # csrc/spatial.hip; fewshot_ds.AUG_REC_INTS: int32 per image record
SPP_REC_INTS = 16            # csrc/spatial.hip; fewshot_ds.SPP_REC_INTS: int32 per instance record


def _gather_from_slots(fn: str, entry: str, slots, desc, expects: str, lut: torch.Tensor, size, size_name: str,
                       with_mask: bool = False):
    """The wrapper of the gathers from source slots into a stem input (``fn``, over the library's ``entry``).  ``slots``:
    (name, uint8 [n,capacity]) pairs, row i the bytes of item i; ``desc`` = (name, int32 [n,ints] ON THE DEVICE, ints):
    what the kernel reads about every item; ``lut`` [3,256]; ``size``: (H, W), or (S,) for a square output.  -> fp32
    [n,H,W,4], ``with_mask`` also uint8 [n,H,W]."""
    for name, t in slots:
        _chk(t, name, torch.uint8)
    desc_name, desc, desc_ints = desc
    _chk(desc, desc_name, torch.int32)
    _chk(lut, 'lut')
    src = slots[0][1]
    n = src.shape[0] if src.dim() == 2 else -1
    if n < 0 or tuple(desc.shape) != (n, desc_ints) or desc.device != src.device or \
            any(t.dim() != 2 or t.shape[0] != n or t.device != src.device for _, t in slots[1:]):
        raise _lib.FgnHipError(f'{fn}: expects {expects} on one device')
    if tuple(lut.shape) != (3, 256) or lut.device != src.device:
        raise _lib.FgnHipError(f'{fn}: lut must be [3,256] on the device of src')
    size = tuple(int(v) for v in size)
    if not all(0 <= v <= RESIZE_MAX_DIM for v in size):
        raise _lib.FgnHipError(f'{fn}: {size_name} must be within 0..{RESIZE_MAX_DIM}, '
                               f'got {size if len(size) > 1 else size[0]}')
    hw = size if len(size) > 1 else size * 2
    y = torch.empty((n,) + hw + (4,), device=src.device, dtype=torch.float32)
    m = torch.empty((n,) + hw, device=src.device, dtype=torch.uint8) if with_mask else None
    if y.numel():                       # (an empty tensor has no address to hand over)
        # (capacity 0: every item is refused by the kernel; it needs an address only)
        slots = [t if t.shape[1] else t.new_zeros((n, 1)) for _, t in slots]
        args = [a for t in slots for a in (_ptr(t), int(t.shape[1]))] + [_ptr(desc), _ptr(lut), _ptr(y)]
        _lib.check(getattr(_lib.load(), entry)(*args, *([_ptr(m)] if with_mask else []), n, *size, _stream()), entry)
    return (y, m) if with_mask else y


def resize_u8_to_nhwc4(src: torch.Tensor, src_hw: torch.Tensor, lut: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """Source-size images -> the NHWC4 fp32 stem input at (H, W): ``u8hwc3_to_nhwc4`` of
    ``fewshot_ds.resize_image_u8`` of every image, bit for bit.  ``src`` uint8 [n, capacity]: image b is
    [h_b, w_b, 3] pixels at the start of row b; ``src_hw`` int32 [n,2] ON THE DEVICE holds (h_b, w_b) and is read by
    the kernel (the launch is the same for every source size).  An image whose size is outside 1..16384 or exceeds the
    capacity comes out as zeros."""
    return _gather_from_slots('resize_u8_to_nhwc4', 'fgn_resize_u8hwc3_to_nhwc4_f32', [('src', src)],
                              ('src_hw', src_hw, 2), 'src [n,capacity] and src_hw [n,2]', lut, (H, W), 'output size')


def augment_u8_to_nhwc4(src: torch.Tensor, recs: torch.Tensor, lut: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """Source-size images -> the augmented NHWC4 fp32 stem input at (H, W): ``u8hwc3_to_nhwc4`` of
    ``fewshot_ds.augment_image_u8`` of every image, bit for bit, in one launch.  ``src`` as for ``resize_u8_to_nhwc4``;
    ``recs`` int32 [n,16] ON THE DEVICE: the records of ``fewshot_ds.query_augment_record``, read by the kernel (the
    launch is the same for every source size and augmentation).  An image whose record is out of range or whose size
    exceeds the capacity comes out as zeros."""
    return _gather_from_slots('augment_u8_to_nhwc4', 'fgn_augment_u8hwc3_to_nhwc4_f32', [('src', src)],
                              ('recs', recs, AUG_REC_INTS), 'src [n,capacity] and recs [n,16]', lut, (H, W),
                              'output size')


def support_from_source(src: torch.Tensor, msk: torch.Tensor, recs: torch.Tensor, lut: torch.Tensor, S: int):
    """Image and mask windows of n support instances -> (the NHWC4 fp32 stem input [n,S,S,4], the support masks
    uint8 0/1 [n,S,S]): ``u8hwc3_to_nhwc4`` of ``fewshot_ds.support_from_source``'s crop and its mask, bit for bit, in
    one launch.  ``src`` uint8 [n, capacity]: instance i's window [wh_i, ww_i, 3] at the start of row i; ``msk`` uint8
    [n, mask capacity]: its mask window [wh_i, ww_i] (nonzero = set); ``recs`` int32 [n,16] ON THE DEVICE: the records
    of ``fewshot_ds.support_geometry``, read by the kernel (the launch is the same for every support set).  An instance
    whose record is out of range or whose window exceeds a capacity comes out as padding with an empty mask."""
    return _gather_from_slots('support_from_source', 'fgn_support_from_source_f32', [('src', src), ('msk', msk)],
                              ('recs', recs, SPP_REC_INTS), 'src [n,capacity], msk [n,mask capacity] and recs [n,16]', lut,
                              (S,), 'S', with_mask=True)


def support_from_source_u8(src: torch.Tensor, msk: torch.Tensor, recs: torch.Tensor, S: int):
    """``support_from_source`` with the crops as BYTES: -> (uint8 [n,S,S,3], the support masks uint8 0/1 [n,S,S]) =
    ``fewshot_ds.support_from_source``'s crop and mask themselves, bit for bit, in one launch; no table.  Arguments and
    the treatment of a bad record as for ``support_from_source`` (the padding and a refused instance are byte 0).  The
    crops feed ``photometric_u8`` (as [n, 3*S*S] slots) and ``support_augment``."""
    for name, t in (('src', src), ('msk', msk)):
        _chk(t, name, torch.uint8)
    _chk(recs, 'recs', torch.int32)
    n = src.shape[0] if src.dim() == 2 else -1
    if n < 0 or msk.dim() != 2 or msk.shape[0] != n or tuple(recs.shape) != (n, SPP_REC_INTS) or \
            msk.device != src.device or recs.device != src.device:
        raise _lib.FgnHipError('support_from_source_u8: expects src [n,capacity], msk [n,mask capacity] and recs [n,16] '
                               'on one device')
    S = int(S)
    if not 0 <= S <= RESIZE_MAX_DIM:
        raise _lib.FgnHipError(f'support_from_source_u8: S must be within 0..{RESIZE_MAX_DIM}, got {S}')
    crop = torch.empty((n, S, S, 3), device=src.device, dtype=torch.uint8)
    m = torch.empty((n, S, S), device=src.device, dtype=torch.uint8)
    if crop.numel():                    # (an empty tensor has no address to hand over)
        # (capacity 0: every item is refused by the kernel; it needs an address only)
        src, msk = (t if t.shape[1] else t.new_zeros((n, 1)) for t in (src, msk))
        _lib.check(_lib.load().fgn_support_from_source_u8(_ptr(src), int(src.shape[1]), _ptr(msk), int(msk.shape[1]),
                                                          _ptr(recs), _ptr(crop), _ptr(m), n, S, _stream()),
                   'fgn_support_from_source_u8')
    return crop, m


def support_augment(crop: torch.Tensor, msk: torch.Tensor, recs: torch.Tensor, lut: torch.Tensor, S: int):
    """n support crops and their masks -> (the augmented NHWC4 fp32 stem input [n,S,S,4], the augmented masks uint8 0/1
    [n,S,S]): ``u8hwc3_to_nhwc4`` of ``fewshot_ds.augment_image_u8`` and ``fewshot_ds.augment_masks`` at S -> S of
    every instance, bit for bit, in ONE launch (``get_support`` with ``augment_spp``, base_fst.py:1151-1153).  ``crop``
    uint8 [n,S,S,3] and ``msk`` uint8 / bool [n,S,S] (nonzero = set) as ``support_from_source_u8`` makes them; ``recs``
    int32 [n,16] ON THE DEVICE: the records of ``fewshot_ds.query_augment_record(row, (S,S), (S,S))``, read by the kernel.
    An instance whose record is out of range or for another size than S comes out as padding with an empty mask."""
    if msk.dtype == torch.bool:
        msk = msk.view(torch.uint8)
    _chk(crop, 'crop', torch.uint8)
    _chk(msk, 'msk', torch.uint8)
    _chk(recs, 'recs', torch.int32)
    _chk(lut, 'lut')
    S = int(S)
    if not 0 <= S <= RESIZE_MAX_DIM:
        raise _lib.FgnHipError(f'support_augment: S must be within 0..{RESIZE_MAX_DIM}, got {S}')
    n = crop.shape[0] if crop.dim() == 4 else -1
    if n < 0 or tuple(crop.shape) != (n, S, S, 3) or tuple(msk.shape) != (n, S, S) or \
            tuple(recs.shape) != (n, AUG_REC_INTS) or msk.device != crop.device or recs.device != crop.device:
        raise _lib.FgnHipError(f'support_augment: expects crop [n,{S},{S},3], msk [n,{S},{S}] and recs [n,16] on one '
                               f'device')
    if tuple(lut.shape) != (3, 256) or lut.device != crop.device:
        raise _lib.FgnHipError('support_augment: lut must be [3,256] on the device of crop')
    y = torch.empty((n, S, S, 4), device=crop.device, dtype=torch.float32)
    m = torch.empty((n, S, S), device=crop.device, dtype=torch.uint8)
    if y.numel():                       # (an empty tensor has no address to hand over)
        _lib.check(_lib.load().fgn_support_augment_f32(_ptr(crop), _ptr(msk), _ptr(recs), _ptr(lut), _ptr(y), _ptr(m),
                                                       n, S, _stream()), 'fgn_support_augment_f32')
    return y, m


def _gather_masks(fn: str, entry: str, masks: torch.Tensor, rec: Optional[torch.Tensor], H: int, W: int) -> torch.Tensor:
    """The wrapper of the two mask gathers (``fn``, over the library's ``entry``): masks [G,h,w] bool / uint8, with or
    without the record of their image -> uint8 0/1 [G,H,W]."""
    if masks.dtype == torch.bool:
        masks = masks.view(torch.uint8)
    _chk(masks, 'masks', torch.uint8)
    if rec is not None:
        _chk(rec, 'rec', torch.int32)
    if masks.dim() != 3:
        raise _lib.FgnHipError(f'{fn}: masks must be [G,h,w]')
    if rec is not None and (tuple(rec.shape) != (AUG_REC_INTS,) or rec.device != masks.device):
        raise _lib.FgnHipError(f'{fn}: rec must be int32 [16] on the device of masks')
    g, h, w = masks.shape
    H, W = int(H), int(W)
    if not (0 <= H <= RESIZE_MAX_DIM and 0 <= W <= RESIZE_MAX_DIM and h <= RESIZE_MAX_DIM and w <= RESIZE_MAX_DIM):
        raise _lib.FgnHipError(f'{fn}: every dimension must be at most {RESIZE_MAX_DIM}')
    out = torch.empty((g, H, W), device=masks.device, dtype=torch.uint8)
    if out.numel() == 0:
        return out
    if h == 0 or w == 0:
        raise _lib.FgnHipError(f'{fn}: empty source masks')
    _lib.check(getattr(_lib.load(), entry)(_ptr(masks), _ptr(out), *([] if rec is None else [_ptr(rec)]), g, h, w, H, W,
                                           _stream()), entry)
    return out


def resize_masks(masks: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """Dense binary masks [G,h,w] (bool / uint8, non-zero = set) -> uint8 0/1 [G,H,W]: ``fewshot_ds.resize_masks`` bit
    for bit (the ground-truth side of the query resize)."""
    return _gather_masks('resize_masks', 'fgn_resize_mask_u8', masks, None, H, W)


def augment_masks(masks: torch.Tensor, rec: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """Dense binary masks [G,h,w] (bool / uint8, non-zero = set) of one image -> uint8 0/1 [G,H,W] by the image's record
    ``rec`` (int32 [16] ON THE DEVICE): ``fewshot_ds.augment_masks`` bit for bit.  A record out of range, or one for
    another source size, gives empty masks."""
    if rec is None:
        raise _lib.FgnHipError('augment_masks: rec must be int32 [16] on the device of masks')
    return _gather_masks('augment_masks', 'fgn_augment_mask_u8', masks, rec, H, W)


PHOTO_REC_INTS = 64          # csrc/spatial.hip; fewshot_ds.PHOTO_REC_INTS: int32 per image record


def photometric_u8(src: torch.Tensor, recs: torch.Tensor) -> torch.Tensor:
    """Source-size images -> the same slots after their photometric operator: ``fewshot_ds.photometric_image_u8`` of
    every image, bit for bit, in one launch.  ``src`` uint8 [n,capacity] as for ``resize_u8_to_nhwc4``; ``recs`` int32
    [n,64] ON THE DEVICE: the records of ``fewshot_ds.query_photometric_record``, read by the kernel.  -> a new uint8
    [n,capacity]: the h * w * 3 bytes of every image are written, what lies behind them in a slot is not.  An image whose
    record is out of range or whose size exceeds the capacity has its slot written as zeros."""
    _chk(src, 'src', torch.uint8)
    _chk(recs, 'recs', torch.int32)
    if src.dim() != 2 or tuple(recs.shape) != (src.shape[0], PHOTO_REC_INTS) or recs.device != src.device:
        raise _lib.FgnHipError('photometric_u8: expects src [n,capacity] and recs [n,64] on one device')
    dst = torch.empty_like(src)
    if src.numel() == 0:                # (an empty tensor has no address to hand over)
        return dst
    _lib.check(_lib.load().fgn_photometric_u8hwc3(_ptr(src), _ptr(dst), int(src.shape[1]), _ptr(recs),
                                                  int(src.shape[0]), _stream()), 'fgn_photometric_u8hwc3')
    return dst


PHOTO_CHAIN_MAX = 3          # csrc/spatial.hip; fewshot_ds.PHOTO_CHAIN_MAX: records per image of a chain


def photometric_chain_u8(src: torch.Tensor, recs: torch.Tensor) -> torch.Tensor:
    """``photometric_u8`` for a chain of operators per image: ``fewshot_ds.photometric_chain_u8`` (the left fold of
    ``photometric_image_u8`` over the image's records) of every image, bit for bit, in ONE launch that reads and writes
    every image once.  ``recs`` int32 [n,P,64] ON THE DEVICE, P in 1..3: the records of
    ``fewshot_ds.photometric_chain_records`` - point operators, then at most one blur.  -> a new uint8 [n,capacity].  An
    image with a record out of range, records of differing (h, w) or an active record behind a blur has its slot written
    as zeros."""
    _chk(src, 'src', torch.uint8)
    _chk(recs, 'recs', torch.int32)
    if src.dim() != 2 or recs.dim() != 3 or not 1 <= recs.shape[1] <= PHOTO_CHAIN_MAX or \
            (recs.shape[0], recs.shape[2]) != (src.shape[0], PHOTO_REC_INTS) or recs.device != src.device:
        raise _lib.FgnHipError(f'photometric_chain_u8: expects src [n,capacity] and recs [n,P,64] with P in 1..'
                               f'{PHOTO_CHAIN_MAX} on one device')
    dst = torch.empty_like(src)
    if src.numel() == 0:                # (an empty tensor has no address to hand over)
        return dst
    _lib.check(_lib.load().fgn_photometric_chain_u8hwc3(_ptr(src), _ptr(dst), int(src.shape[1]), _ptr(recs),
                                                        int(recs.shape[1]), int(src.shape[0]), _stream()),
               'fgn_photometric_chain_u8hwc3')
    return dst


def maxpool3x3s2(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk(x, 'x')
    n, h, w, c = x.shape
    shape = (n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c)
    if out is None:
        y = torch.empty(shape, device=x.device, dtype=torch.float32)
    else:
        _chk(out, 'out')
        if tuple(out.shape) != shape:
            raise _lib.FgnHipError('maxpool3x3s2: bad out shape')
        y = out
    _lib.check(_lib.load().fgn_maxpool3x3s2_nhwc_f32(_ptr(x), _ptr(y), n, h, w, c, _stream()),
               'fgn_maxpool3x3s2_nhwc_f32')
    return y


def group_norm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float = 1e-5,
               relu: bool = False, residual: Optional[torch.Tensor] = None, inplace: bool = False) -> torch.Tensor:
    """torch.nn.GroupNorm over NHWC x [n,H,W,C] (+ residual) (+ ReLU)."""
    _chk(x, 'x')
    _chk(gamma, 'gamma')
    _chk(beta, 'beta')
    n, h, w, c = x.shape
    if gamma.numel() != c or beta.numel() != c or c % groups != 0:
        raise _lib.FgnHipError('group_norm: bad gamma/beta/groups')
    if residual is not None:
        _chk(residual, 'residual')
        if residual.shape != x.shape:
            raise _lib.FgnHipError('group_norm: bad residual shape')
    lib = _lib.load()
    nbytes = lib.fgn_group_norm_workspace_bytes(n, h * w, c, groups)
    ws = torch.empty(max(nbytes // 8, 1), device=x.device, dtype=torch.float64)
    y = x if inplace else torch.empty_like(x)
    _lib.check(lib.fgn_group_norm_nhwc_f32(_ptr(x), _ptr(y), _ptr(gamma), _ptr(beta), _ptr(residual), _ptr(ws), nbytes,
                                           n, h * w, c, groups, float(eps), int(relu), _stream()),
               'fgn_group_norm_nhwc_f32')
    return y


def avgpool2x2(x: torch.Tensor) -> torch.Tensor:
    """AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False) over NHWC."""
    _chk(x, 'x')
    n, h, w, c = x.shape
    y = torch.empty((n, (h + 1) // 2, (w + 1) // 2, c), device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().fgn_avgpool2x2_nhwc_f32(_ptr(x), _ptr(y), n, h, w, c, _stream()), 'fgn_avgpool2x2_nhwc_f32')
    return y


def roi_align(fmap: torch.Tensor, rois: torch.Tensor, out_size: int, spatial_scale: float,
              sampling_ratio: int, aligned: bool, n_rois_dev: Optional[torch.Tensor] = None,
              post_shift: Optional[torch.Tensor] = None, relu: bool = False,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fmap [B,H,W,C], rois [R,5] -> [R,P,P,C] (+ post_shift[C], ReLU)."""
    _chk(fmap, 'fmap')
    _chk(rois, 'rois')
    b, h, w, c = fmap.shape
    if post_shift is not None:
        _chk(post_shift, 'post_shift')
        if post_shift.numel() != c:
            raise _lib.FgnHipError('roi_align: post_shift must be [C]')
    if rois.dim() != 2 or rois.shape[1] != 5:
        raise _lib.FgnHipError('roi_align: rois must be [R,5]')
    r = rois.shape[0]
    if out is None:
        out = torch.empty((r, out_size, out_size, c), device=fmap.device, dtype=torch.float32)
    else:
        _chk(out, 'out')
        if tuple(out.shape) != (r, out_size, out_size, c):
            raise _lib.FgnHipError('roi_align: bad out shape')
    if n_rois_dev is not None:
        _chk(n_rois_dev, 'n_rois_dev', torch.int32)
    rc = _lib.load().fgn_roi_align_nhwc_f32(_ptr(fmap), _ptr(rois), _ptr(out), _ptr(n_rois_dev), r, b, h, w, c,
                                            out_size, float(spatial_scale), sampling_ratio, int(aligned),
                                            _ptr(post_shift), int(relu), _stream())
    _lib.check(rc, 'fgn_roi_align_nhwc_f32')
    return out


def roi_align2(fmap: torch.Tensor, fmap2: torch.Tensor, rois: torch.Tensor, out_size: int, spatial_scale: float,
               sampling_ratio: int, aligned: bool, n_rois_dev: Optional[torch.Tensor] = None,
               post_shift2: Optional[torch.Tensor] = None, relu2: bool = False):
    """Two maps of one spatial size pooled at the same RoIs by ONE launch: -> ([R,P,P,C], [R,P,P,C2] (+ post_shift2,
    ReLU)); identical bytes to two ``roi_align`` calls."""
    _chk(fmap, 'fmap')
    _chk(fmap2, 'fmap2')
    _chk(rois, 'rois')
    b, h, w, c = fmap.shape
    c2 = fmap2.shape[3]
    if tuple(fmap2.shape[:3]) != (b, h, w) or rois.dim() != 2 or rois.shape[1] != 5:
        raise _lib.FgnHipError('roi_align2: operand shapes inconsistent')
    if post_shift2 is not None:
        _chk(post_shift2, 'post_shift2')
        if post_shift2.numel() != c2:
            raise _lib.FgnHipError('roi_align2: post_shift2 must be [C2]')
    if n_rois_dev is not None:
        _chk(n_rois_dev, 'n_rois_dev', torch.int32)
    r = rois.shape[0]
    out = torch.empty((r, out_size, out_size, c), device=fmap.device, dtype=torch.float32)
    out2 = torch.empty((r, out_size, out_size, c2), device=fmap.device, dtype=torch.float32)
    rc = _lib.load().fgn_roi_align2_nhwc_f32(_ptr(fmap), _ptr(fmap2), _ptr(rois), _ptr(out), _ptr(out2), _ptr(n_rois_dev),
                                             r, b, h, w, c, c2, out_size, float(spatial_scale), sampling_ratio,
                                             int(aligned), _ptr(post_shift2), int(relu2), _stream())
    _lib.check(rc, 'fgn_roi_align2_nhwc_f32')
    return out, out2


def roi_align_mask(mask_u8: torch.Tensor, rois: torch.Tensor, out_size: int, spatial_scale: float,
                   sampling_ratio: int, aligned: bool) -> torch.Tensor:
    """mask [B,H,W] uint8 -> [R,P,P] fp32."""
    _chk(mask_u8, 'mask', torch.uint8)
    _chk(rois, 'rois')
    b, h, w = mask_u8.shape
    r = rois.shape[0]
    out = torch.empty((r, out_size, out_size), device=mask_u8.device, dtype=torch.float32)
    rc = _lib.load().fgn_roi_align_mask_u8(_ptr(mask_u8), _ptr(rois), _ptr(out), r, b, h, w, out_size,
                                           float(spatial_scale), sampling_ratio, int(aligned), _stream())
    _lib.check(rc, 'fgn_roi_align_mask_u8')
    return out


def support_class_vectors(x: torch.Tensor, weights: Optional[torch.Tensor], n_groups: int, k: int) -> torch.Tensor:
    """x [n_groups*k, P.., C] -> [n_groups, C] mean over (k, P) of x * weights."""
    _chk(x, 'x')
    c = x.shape[-1]
    p = x[0].numel() // c
    if x.shape[0] != n_groups * k:
        raise _lib.FgnHipError('support_class_vectors: leading dim != n_groups*k')
    if weights is not None:
        _chk(weights, 'weights')
        if weights.numel() != n_groups * k * p:
            raise _lib.FgnHipError('support_class_vectors: weights shape mismatch')
    out = torch.empty((n_groups, c), device=x.device, dtype=torch.float32)
    rc = _lib.load().fgn_support_class_vectors_f32(_ptr(x), _ptr(weights), _ptr(out), n_groups, k, p, c, _stream())
    _lib.check(rc, 'fgn_support_class_vectors_f32')
    return out


def scale_channels(x: torch.Tensor, v: torch.Tensor, div: int) -> torch.Tensor:
    """x [n_in, ..., C], v [n_in*div, C] -> [n_in*div, ..., C] = x[n // div] * v[n]."""
    _chk(x, 'x')
    _chk(v, 'v')
    n_out, c = v.shape
    if x.shape[0] * div != n_out or x.shape[-1] != c:
        raise _lib.FgnHipError('scale_channels: operand shapes inconsistent')
    out = torch.empty((n_out,) + tuple(x.shape[1:]), device=x.device, dtype=torch.float32)
    p = math.prod(x.shape[1:-1])
    _lib.check(_lib.load().fgn_scale_channels_f32(_ptr(x), _ptr(v), _ptr(out), n_out, div, p, c, _stream()),
               'fgn_scale_channels_f32')
    return out


def support_kmean(x: torch.Tensor, n_groups: int, k: int) -> torch.Tensor:
    _chk(x, 'x')
    if x.shape[0] != n_groups * k:
        raise _lib.FgnHipError('support_kmean: leading dim != n_groups*k')
    c = x.shape[-1]
    p = x[0].numel() // c
    out = torch.empty((n_groups,) + tuple(x.shape[1:]), device=x.device, dtype=torch.float32)
    rc = _lib.load().fgn_support_kmean_f32(_ptr(x), _ptr(out), n_groups, k, p, c, _stream())
    _lib.check(rc, 'fgn_support_kmean_f32')
    return out


def gather_support_vectors(table: torch.Tensor, labels: torch.Tensor, rois: Optional[torch.Tensor],
                           n_ways: int, n_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk(table, 'table')
    _chk(labels, 'labels', torch.int64)
    n, c = labels.shape[0], table.shape[-1]
    if rois is not None:
        _chk(rois, 'rois')
        if rois.shape[0] < n or rois.shape[1] != 5:
            raise _lib.FgnHipError('gather_support_vectors: rois must be [>=n,5]')
    out = zeros((n, c), table.device)
    rc = _lib.load().fgn_gather_support_vectors_f32(_ptr(table), _ptr(labels), _ptr(rois), _ptr(out), _ptr(n_dev),
                                                    n, n_ways, c, _stream())
    _lib.check(rc, 'fgn_gather_support_vectors_f32')
    return out


def relation_gn_head(q: torch.Tensor, s: torch.Tensor, rois: torch.Tensor, gn_w, gn_b, fc_w, fc_b,
                     n_ways: int, gn_groups: int, eps: float, n_rois_dev: Optional[torch.Tensor] = None,
                     rel_out: Optional[torch.Tensor] = None):
    """q [R,7,7,C]; s [B*N,7,7,C]; rois [R,5] -> cls_raw [R*N,2], reg_raw [R*N,4].  ``rel_out`` (parity tests):
    [R*N,7,7,C] receives the relation feature map the reference materialises (fgn_roi_head.py:274)."""
    for t, nm in ((q, 'Q'), (s, 'S'), (rois, 'rois'), (gn_w, 'gn_w'), (gn_b, 'gn_b'), (fc_w, 'fc_w'), (fc_b, 'fc_b')):
        _chk(t, nm)
    r, p, _, c = q.shape
    if s.shape[1:] != q.shape[1:] or s.shape[0] % n_ways or rois.shape[0] < r or fc_w.shape != (6, c):
        raise _lib.FgnHipError('relation_gn_head: operand shapes inconsistent')
    if rel_out is not None:
        _chk(rel_out, 'rel_out')
        if tuple(rel_out.shape) != (r * n_ways, p, p, c):
            raise _lib.FgnHipError('relation_gn_head: rel_out must be [R*N,P,P,C]')
    cls = zeros((r * n_ways, 2), q.device)
    reg = zeros((r * n_ways, 4), q.device)
    L = _lib.load()
    scratch = torch.empty(L.fgn_relation_gn_head_scratch_bytes(r, n_ways, c), device=q.device, dtype=torch.uint8)
    rc = L.fgn_relation_gn_head_f32(_ptr(q), _ptr(s), _ptr(rois), _ptr(gn_w), _ptr(gn_b), _ptr(fc_w),
                                    _ptr(fc_b), _ptr(cls), _ptr(reg), _ptr(n_rois_dev), r, n_ways, c,
                                    gn_groups, p, float(eps), _ptr(rel_out), _ptr(scratch), _stream())
    _lib.check(rc, 'fgn_relation_gn_head_f32')
    return cls, reg


# --------------------------------------------------------------------------------------
# selection stages
# --------------------------------------------------------------------------------------
MAX_RATIO = float(np.float32(abs(math.log(16.0 / 1000.0))))


def base_anchors(scales, ratios, base_size) -> np.ndarray:
    """mmdet AnchorGenerator base anchors (ratio-major, centre 0, not rounded), fp32."""
    f = np.float32
    w = h = f(base_size)
    ratios = np.asarray(ratios, f)
    scales = np.asarray(scales, f)
    h_ratios = np.sqrt(ratios)
    w_ratios = (f(1) / h_ratios).astype(f)
    ws = (w * w_ratios[:, None] * scales[None, :]).reshape(-1).astype(f)
    hs = (h * h_ratios[:, None] * scales[None, :]).reshape(-1).astype(f)
    c = f(0.0) * w
    return np.stack([c - f(0.5) * ws, c - f(0.5) * hs, c + f(0.5) * ws, c + f(0.5) * hs], -1).astype(f)


def rpn_merge(head: torch.Tensor, batch: int, n_ways: int, n_anchors: int):
    """head [B*N, h, w, CH] -> logits, scores [B, h*w*A], deltas [B, h*w*A, 4]."""
    _chk(head, 'head')
    bn, h, w, ch = head.shape
    if bn != batch * n_ways:
        raise _lib.FgnHipError('rpn_merge: leading dim != batch*n_ways')
    n = h * w * n_anchors
    logits = torch.empty((batch, n), device=head.device, dtype=torch.float32)
    scores = torch.empty_like(logits)
    deltas = torch.empty((batch, n, 4), device=head.device, dtype=torch.float32)
    rc = _lib.load().fgn_rpn_merge_f32(_ptr(head), _ptr(logits), _ptr(scores), _ptr(deltas), batch, n_ways, h * w,
                                       n_anchors, ch, _stream())
    _lib.check(rc, 'fgn_rpn_merge_f32')
    return logits, scores, deltas


def rpn_proposals(scores: torch.Tensor, deltas: torch.Tensor, anchors_base: torch.Tensor, feat_h: int, feat_w: int,
                  stride: int, img_h: int, img_w: int, means, stds, nms_pre: int, min_bbox_size: float,
                  iou_thr: float, max_per_img: int, debug_topk: bool = False, with_rois: bool = False,
                  with_info: bool = False):
    """-> proposals [B,max_per_img,5] (x1,y1,x2,y2,score), n_props [B] int32 (+ with_rois: the same boxes as
    [B*max_per_img,5] RoIs (image index, box) = bbox2roi, fgn_roi_head.py:556; + with_info, last: the [B,8] int32
    info words of the multi-workgroup pre-selection - b1, count before b1, b2, candidate count, ok flag, finished by
    rpn_matrix_nms_kernel - all zero when the pre-selection is not launched; like debug_topk it keeps the call off the
    training-size route, which has no such words)."""
    _chk(scores, 'scores')
    _chk(deltas, 'deltas')
    _chk(anchors_base, 'anchors_base')
    batch, n_total = scores.shape
    a = anchors_base.shape[0]
    if n_total != feat_h * feat_w * a or tuple(deltas.shape) != (batch, n_total, 4):
        raise _lib.FgnHipError('rpn_proposals: operand shapes inconsistent')
    L = _lib.load()
    props = torch.empty((batch, max_per_img, 5), device=scores.device, dtype=torch.float32)
    rois = torch.empty((batch * max_per_img, 5), device=scores.device, dtype=torch.float32)   # bbox2roi of the proposals
    n_props = zeros((batch,), scores.device, torch.int32)
    n_sel = nms_pre if 0 < nms_pre < n_total else n_total
    if (n_sel > 8192 or max_per_img > 1024) and not (debug_topk or with_info):
        # training sizes (train_cfg.rpn_proposal: 12000 -> 2000): the ranking runs as a global sort over many workgroups
        scratch = torch.empty(L.fgn_rpn_proposals_large_scratch_bytes(batch, n_total, nms_pre), device=scores.device,
                              dtype=torch.uint8)
        rc = L.fgn_rpn_proposals_large_f32(_ptr(scores), _ptr(deltas), _ptr(anchors_base), _ptr(scratch), _ptr(props),
                                           _ptr(rois), _ptr(n_props), batch, feat_h, feat_w, a, stride, float(img_h),
                                           float(img_w), _f4(means), _f4(stds), MAX_RATIO, nms_pre,
                                           float(min_bbox_size), float(iou_thr), max_per_img, _stream())
        _lib.check(rc, 'fgn_rpn_proposals_large_f32')
        return (props, n_props, rois) if with_rois else (props, n_props)
    scratch = torch.empty(L.fgn_rpn_proposals_scratch_bytes(batch, n_total, nms_pre), device=scores.device,
                          dtype=torch.uint8)
    dbg = None
    if debug_topk:
        dbg = torch.full((batch, 8192), -1, device=scores.device, dtype=torch.int32)
    # zero-filled workspace of the multi-workgroup pre-selection (histograms, counters): from the episode's zero arena
    pre_zeroed = zeros((L.fgn_rpn_proposals_zeroed_bytes(batch),), scores.device, torch.uint8)
    rc = L.fgn_rpn_proposals_f32(_ptr(scores), _ptr(deltas), _ptr(anchors_base), _ptr(scratch), _ptr(pre_zeroed),
                                 _ptr(props), _ptr(rois), _ptr(n_props), _ptr(dbg), batch, feat_h, feat_w, a, stride,
                                 float(img_h),
                                 float(img_w), _f4(means), _f4(stds), MAX_RATIO, nms_pre, float(min_bbox_size),
                                 float(iou_thr), max_per_img, _stream())
    _lib.check(rc, 'fgn_rpn_proposals_f32')
    out = (props, n_props)
    if debug_topk:
        out += (dbg,)
    elif with_rois:
        out += (rois,)
    if with_info:
        # (fgn_rpn_proposals_f32 lays the workspace out as hist1 [B][4096] | hist2 [B][4096] | info [B][8] | counter [B])
        out += (pre_zeroed[batch * 2 * 4096 * 4:batch * (2 * 4096 * 4 + 32)].view(torch.int32).view(batch, 8),)
    return out


def det_post(rois: torch.Tensor, cls_raw: torch.Tensor, reg_raw: torch.Tensor, n_ways: int, img_h: int, img_w: int,
             means, stds, score_thr: float, iou_thr: float, max_per_img: int,
             n_rois_dev: Optional[torch.Tensor] = None, debug_scores: bool = False, img_index: Optional[int] = None,
             batch: int = 1, out=None):
    """-> det [max_per_img,5], labels, n_det (+ with ``img_index``: mask RoIs [max_per_img,5] = (img_index, box), the
    mask branch's bbox2roi, fgn_roi_head.py:654).  ``batch`` > 1: the RoIs of ``batch`` images stacked ([batch*R,5],
    ``n_rois_dev`` [batch] when given), one workgroup per image in one launch; outputs stacked the same way
    ([batch*max_per_img,5], ..., n_det [batch]), image i carrying index ``img_index + i``.  ``out``: caller-owned
    (det, labels, n_det) of those shapes, n_det ZERO on entry (the packed result record of the detector)."""
    for t, nm in ((rois, 'rois'), (cls_raw, 'cls_raw'), (reg_raw, 'reg_raw')):
        _chk(t, nm)
    if batch < 1 or rois.shape[0] % batch:
        raise _lib.FgnHipError('det_post: the RoI rows are not a multiple of batch')
    r = rois.shape[0] // batch
    if rois.shape[1] != 5 or tuple(cls_raw.shape) != (batch * r * n_ways, 2) or \
            tuple(reg_raw.shape) != (batch * r * n_ways, 4):
        raise _lib.FgnHipError('det_post: operand shapes inconsistent')
    if n_rois_dev is not None and n_rois_dev.numel() < batch:
        raise _lib.FgnHipError('det_post: n_rois_dev holds fewer counts than batch')
    L = _lib.load()
    scratch = torch.empty(batch * L.fgn_det_post_scratch_bytes(r, n_ways), device=rois.device, dtype=torch.uint8)
    if out is not None:
        det, lab, n_det = out
        _chk(det, 'out det'); _chk(lab, 'out labels', torch.int64); _chk(n_det, 'out n_det', torch.int32)
        if tuple(det.shape) != (batch * max_per_img, 5) or tuple(lab.shape) != (batch * max_per_img,) or n_det.numel() != batch:
            raise _lib.FgnHipError('det_post: bad out shapes')
    else:
        det = torch.empty((batch * max_per_img, 5), device=rois.device, dtype=torch.float32)
        lab = torch.empty((batch * max_per_img,), device=rois.device, dtype=torch.int64)
        n_det = zeros((batch,), rois.device, torch.int32)
    mrois = torch.empty((batch * max_per_img, 5), device=rois.device, dtype=torch.float32) \
        if img_index is not None else None
    # softmax scores [r, n_ways + 1] of the first image followed by 16 words of phase stamps (tools/post_time.py)
    dbg = torch.zeros((r * (n_ways + 1) + 16,), device=rois.device, dtype=torch.float32) if debug_scores else None
    rc = L.fgn_det_post_f32(_ptr(rois), _ptr(cls_raw), _ptr(reg_raw), _ptr(n_rois_dev), _ptr(scratch), _ptr(det),
                            _ptr(mrois), int(img_index or 0), _ptr(lab), _ptr(n_det), _ptr(dbg), batch, r, n_ways,
                            float(img_h), float(img_w), _f4(means),
                            _f4(stds), MAX_RATIO, float(score_thr), float(iou_thr), max_per_img, _stream())
    _lib.check(rc, 'fgn_det_post_f32')
    if debug_scores:
        det_post.last_stamps = dbg[r * (n_ways + 1):].view(torch.int32)
        return det, lab, n_det, dbg[:r * (n_ways + 1)].view(r, n_ways + 1)
    if img_index is not None:
        return det, lab, n_det, mrois
    return det, lab, n_det


def mask_logits(x: torch.Tensor, w: torch.Tensor, bias, roi_size: int,
                n_dev: Optional[torch.Tensor] = None, prob_out: Optional[torch.Tensor] = None):
    """x [D, P, P, 4*C] (deconv output, sub-position major) -> logits, prob [D, 2P, 2P].  ``bias``: a float, or a
    one-element device tensor the kernel reads itself (no host read of a parameter a training step has just updated)."""
    _chk(x, 'x')
    _chk(w, 'w')
    d = x.shape[0]
    c = w.numel()
    if x.numel() != d * roi_size * roi_size * 4 * c:
        raise _lib.FgnHipError('mask_logits: x shape inconsistent with weight')
    logits = zeros((d, 2 * roi_size, 2 * roi_size), x.device)
    if prob_out is not None:        # caller-owned, ZERO on entry (rows beyond the device count are not written)
        _chk(prob_out, 'prob_out')
        if tuple(prob_out.shape) != (d, 2 * roi_size, 2 * roi_size):
            raise _lib.FgnHipError('mask_logits: bad prob_out shape')
        prob = prob_out
    else:
        prob = zeros((d, 2 * roi_size, 2 * roi_size), x.device)
    bias_dev = None
    if isinstance(bias, torch.Tensor):
        _chk(bias, 'bias')
        bias_dev, bias = bias, 0.0
    rc = _lib.load().fgn_mask_logits_f32(_ptr(x), _ptr(w), float(bias), _ptr(bias_dev), _ptr(logits), _ptr(prob),
                                         _ptr(n_dev), d, roi_size, c, _stream())
    _lib.check(rc, 'fgn_mask_logits_f32')
    return logits, prob


def mask_paste(prob: torch.Tensor, boxes: torch.Tensor, img_h: int, img_w: int, thr: float,
               n_dev: Optional[torch.Tensor] = None, skip_empty: bool = True) -> torch.Tensor:
    """prob [D, M, M], boxes [D, >=4] (x1,y1,x2,y2 first) -> uint8 [D, H, W].  ``skip_empty``: mmdet's CPU paste
    (inside the integer-expanded box) / False: its CUDA paste (grid over the whole image); equal for thr >= 0.5."""
    _chk(prob, 'prob')
    _chk(boxes, 'boxes')
    d, m, _ = prob.shape
    if boxes.shape[0] != d or boxes.shape[1] < 4:
        raise _lib.FgnHipError('mask_paste: boxes shape mismatch')
    out = torch.empty((d, img_h, img_w), device=prob.device, dtype=torch.uint8)
    rc = _lib.load().fgn_mask_paste_u8(_ptr(prob), _ptr(boxes), boxes.shape[1], _ptr(out), _ptr(n_dev), d, img_h,
                                       img_w, m, float(thr), int(bool(skip_empty)), _stream())
    _lib.check(rc, 'fgn_mask_paste_u8')
    return out


RLE_TRANS_CAP = 16384     # transitions per detection kept on device
RLE_BYTE_CAP = 16384      # COCO string bytes per detection


def mask_rle(prob: torch.Tensor, boxes: torch.Tensor, img_h: int, img_w: int, thr: float,
             n_dev: Optional[torch.Tensor] = None, skip_empty: bool = True, out=None):
    """Fused paste + threshold + COCO RLE.  Returns (bytes [D,RLE_BYTE_CAP] u8, lens [D] i32,
    overflow [D] i32), all on device.  ``out``: caller-owned tensors of those shapes, lens / overflow ZERO on entry."""
    _chk(prob, 'prob')
    _chk(boxes, 'boxes')
    d, m, _ = prob.shape
    if boxes.shape[0] != d or boxes.shape[1] < 4:
        raise _lib.FgnHipError('mask_rle: boxes shape mismatch')
    dev = prob.device
    scratch = torch.empty((d, RLE_TRANS_CAP), device=dev, dtype=torch.int32)
    if out is not None:
        out, lens, ovf = out
        _chk(out, 'out bytes', torch.uint8); _chk(lens, 'out lens', torch.int32); _chk(ovf, 'out overflow', torch.int32)
        if tuple(out.shape) != (d, RLE_BYTE_CAP) or lens.numel() != d or ovf.numel() != d:
            raise _lib.FgnHipError('mask_rle: bad out shapes')
    else:
        out = torch.empty((d, RLE_BYTE_CAP), device=dev, dtype=torch.uint8)
        lens = zeros((d,), dev, torch.int32)
        ovf = zeros((d,), dev, torch.int32)
    rc = _lib.load().fgn_mask_rle(_ptr(prob), _ptr(boxes), boxes.shape[1], _ptr(scratch), _ptr(out), _ptr(lens),
                                  _ptr(ovf), _ptr(n_dev), d, img_h, img_w, m, float(thr), RLE_TRANS_CAP,
                                  RLE_BYTE_CAP, int(bool(skip_empty)), _stream())
    _lib.check(rc, 'fgn_mask_rle')
    return out, lens, ovf


def mask_rle_src(prob: torch.Tensor, boxes: torch.Tensor, src_hw: torch.Tensor, net_hw, thr: float,
                 n_dev: Optional[torch.Tensor] = None, skip_empty: bool = True, out=None, boxes_src_out=None):
    """``mask_rle`` of a whole batch with the results at SOURCE size, one launch: ``prob`` [B*D,M,M] and ``boxes``
    [B*D,>=4] hold D rows per image, the boxes in the frame of the ``net_hw`` = (H, W) network; ``src_hw`` int32 [B,2]
    ON THE DEVICE holds (h_b, w_b) and is read by the kernel (the launch is the same for every source size); ``n_dev``
    int32 [B]: the images' detection counts.  Every box is divided by its image's scale
    (``fewshot_ds.boxes_to_source``, bit for bit) and pasted into h_b x w_b.  Returns (bytes [B*D,RLE_BYTE_CAP] u8,
    lens [B*D] i32, overflow [B*D] i32); ``out``: caller-owned tensors of those sizes, lens / overflow ZERO on entry.
    ``boxes_src_out``: a float32 [B*D,4] tensor that receives the divided boxes.  An image whose size is outside
    1..16384 comes out with lengths 0."""
    _chk(prob, 'prob')
    _chk(boxes, 'boxes')
    _chk(src_hw, 'src_hw', torch.int32)
    rows, m, _ = prob.shape
    dev = prob.device
    if src_hw.dim() != 2 or src_hw.shape[1] != 2 or src_hw.device != dev:
        raise _lib.FgnHipError('mask_rle_src: src_hw must be int32 [B,2] on the device of prob')
    b = int(src_hw.shape[0])
    if boxes.dim() != 2 or boxes.shape[0] != rows or boxes.shape[1] < 4 or (b == 0) != (rows == 0) or (b and rows % b):
        raise _lib.FgnHipError('mask_rle_src: prob / boxes must hold the same number of rows per image of src_hw')
    d = rows // b if b else 0
    if n_dev is not None:
        _chk(n_dev, 'n_dev', torch.int32)
        if n_dev.numel() != b:
            raise _lib.FgnHipError('mask_rle_src: n_dev must hold one count per image')
    H, W = int(net_hw[0]), int(net_hw[1])
    if not (1 <= H <= RESIZE_MAX_DIM and 1 <= W <= RESIZE_MAX_DIM):
        raise _lib.FgnHipError(f'mask_rle_src: the network size must be within 1..{RESIZE_MAX_DIM}, got {(H, W)}')
    if boxes_src_out is not None:
        _chk(boxes_src_out, 'boxes_src_out')
        if tuple(boxes_src_out.shape) != (rows, 4) or boxes_src_out.device != dev:
            raise _lib.FgnHipError('mask_rle_src: boxes_src_out must be float32 [B*D,4] on the device of prob')
    scratch = torch.empty((rows, RLE_TRANS_CAP), device=dev, dtype=torch.int32)
    if out is not None:
        out, lens, ovf = out
        _chk(out, 'out bytes', torch.uint8); _chk(lens, 'out lens', torch.int32); _chk(ovf, 'out overflow', torch.int32)
        if out.numel() != rows * RLE_BYTE_CAP or lens.numel() != rows or ovf.numel() != rows:
            raise _lib.FgnHipError('mask_rle_src: bad out shapes')
    else:
        out = torch.empty((rows, RLE_BYTE_CAP), device=dev, dtype=torch.uint8)
        lens = zeros((rows,), dev, torch.int32)
        ovf = zeros((rows,), dev, torch.int32)
    if rows:
        rc = _lib.load().fgn_mask_rle_src(_ptr(prob), _ptr(boxes), boxes.shape[1], _ptr(src_hw), _ptr(scratch), _ptr(out),
                                          _ptr(lens), _ptr(ovf), _ptr(boxes_src_out), _ptr(n_dev), b, d, H, W, m,
                                          float(thr), RLE_TRANS_CAP, RLE_BYTE_CAP, int(bool(skip_empty)), _stream())
        _lib.check(rc, 'fgn_mask_rle_src')
    return out, lens, ovf


def dense_mask_rle(masks: torch.Tensor, packed: bool = False):
    """COCO RLE of dense binary masks [n,H,W] (bool / uint8) on the device: the ground-truth masks of the query
    (``qry_isegmaps_rle``, fgn.py:298).  Returns (bytes [n,RLE_BYTE_CAP] u8, lens [n] i32, overflow [n] i32).
    ``packed``: the three are views of ONE allocation laid out [lens | overflow | bytes] (one device-to-host copy
    moves them all) and that allocation is returned as a fourth value."""
    if masks.dtype == torch.bool:
        masks = masks.view(torch.uint8)
    _chk(masks, 'masks', torch.uint8)
    if masks.dim() != 3:
        raise _lib.FgnHipError('dense_mask_rle: masks must be [n,H,W]')
    n, h, w = masks.shape
    dev = masks.device
    buf = None
    if packed:
        buf = torch.empty(n * (RLE_BYTE_CAP + 8), device=dev, dtype=torch.uint8)
        buf[:n * 8].zero_()
        lens, ovf = buf[:n * 4].view(torch.int32), buf[n * 4:n * 8].view(torch.int32)
        out = buf[n * 8:].view(n, RLE_BYTE_CAP)
    else:
        out = torch.empty((n, RLE_BYTE_CAP), device=dev, dtype=torch.uint8)
        lens = torch.zeros((n,), device=dev, dtype=torch.int32)
        ovf = torch.zeros((n,), device=dev, dtype=torch.int32)
    if n == 0:
        return (out, lens, ovf, buf) if packed else (out, lens, ovf)
    L = _lib.load()
    nbytes = L.fgn_dense_rle_scratch_bytes(n, h, w, RLE_TRANS_CAP)
    scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    _lib.check(L.fgn_dense_mask_rle(_ptr(masks), _ptr(scratch), nbytes, _ptr(out), _ptr(lens), _ptr(ovf), n, h, w,
                                    RLE_TRANS_CAP, RLE_BYTE_CAP, _stream()), 'fgn_dense_mask_rle')
    return (out, lens, ovf, buf) if packed else (out, lens, ovf)


RLE_REC_INTS = 8             # csrc/mask.hip: {h, w, wy, wx, wh, ww, run0, n_runs} per mask


def _rle_window(m, window) -> tuple:
    _, h, w = m.shape
    wy, wx, wh, ww = (0, 0, h, w) if window is None else (int(v) for v in window)
    if not (1 <= h <= RESIZE_MAX_DIM and 1 <= w <= RESIZE_MAX_DIM):
        raise _lib.FgnHipError(f'rle_decode: mask sizes must be within 1..{RESIZE_MAX_DIM}, got {(h, w)}')
    if not (wy >= 0 and wx >= 0 and wh >= 1 and ww >= 1 and wy + wh <= h and wx + ww <= w):
        raise _lib.FgnHipError(f'rle_decode: window {(wy, wx, wh, ww)} is empty or outside its {h}x{w} mask')
    return wy, wx, wh, ww


def _rle_decode(parts: list, recs: np.ndarray, out: torch.Tensor, stride: int, max_wh: int, max_ww: int) -> None:
    """ONE upload - [recs int32 [n,8] | the run ends uint32 of ``parts`` concatenated] as bytes - and ONE launch of
    ``fgn_rle_decode_u8`` into ``out`` (output i at byte i * stride), on the current stream."""
    ends = np.concatenate(parts) if parts else np.zeros(0, np.uint32)
    n = recs.shape[0]
    blob = torch.from_numpy(np.concatenate([np.ascontiguousarray(recs, np.int32).reshape(-1).view(np.uint8),
                                            np.ascontiguousarray(ends, np.uint32).view(np.uint8)]))
    blob = blob.to(out.device, non_blocking=True)
    base = blob.data_ptr()
    # (no run at all: every record is refused by the kernel; it needs an address only)
    _lib.check(_lib.load().fgn_rle_decode_u8(base + 4 * RLE_REC_INTS * n if ends.size else base, int(ends.size), base,
                                             _ptr(out), int(stride), n, int(max_wh), int(max_ww), _stream()),
               'fgn_rle_decode_u8')


def _masks_front(m, window, out: Optional[torch.Tensor], device, fn: str) -> tuple:
    """The front ``rle_decode_masks`` and ``poly_masks`` share: the window of every mask checked, ``out`` allocated on
    ``device`` (default: the current GPU) or verified.  -> (n, (wy, wx, wh, ww), out)."""
    n = int(m.shape[0])
    window = _rle_window(m, window)
    wh, ww = window[2:]
    if out is None:
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        out = torch.empty((n, wh, ww), device=dev, dtype=torch.uint8)
    else:
        _chk(out, 'out', torch.uint8)
        if tuple(out.shape) != (n, wh, ww):
            raise _lib.FgnHipError(f'{fn}: out is {tuple(out.shape)}, expected {(n, wh, ww)}')
    return n, window, out


def _row_items(slot: torch.Tensor, items: list, fn: str) -> list:
    """The front ``rle_decode_rows`` and ``poly_mask_rows`` share: ``slot`` is uint8 [rows, capacity], contiguous, and
    every item (row, carrier of ONE mask, window) names a row of its own whose window fits the capacity.  -> the items
    as (row, carrier, (wy, wx, wh, ww)), the window checked."""
    _chk(slot, 'slot', torch.uint8)
    if slot.dim() != 2:
        raise _lib.FgnHipError(f'{fn}: slot must be [rows, capacity]')
    rows, cap = slot.shape
    seen, checked = set(), []
    for row, m, window in items:
        if not 0 <= int(row) < rows or int(m.shape[0]) != 1 or int(row) in seen:
            raise _lib.FgnHipError(f'{fn}: row {row} of {rows}: one mask per item, one item per row')
        seen.add(int(row))
        window = _rle_window(m, window)
        if window[2] * window[3] > cap:
            raise _lib.FgnHipError(f'{fn}: a window of {window[2] * window[3]} bytes exceeds the slot capacity {cap}')
        checked.append((int(row), m, window))
    return checked


def rle_decode_masks(m, window=None, out: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """The n masks of an ``rle.RleMasks`` (what ``rle.as_masks`` makes of COCO RLE items) -> dense uint8 0/1 [n,h,w] on
    the device, or [n,wh,ww] for one ``window`` = (wy, wx, wh, ww) of every mask: ``rle.decode`` bit for bit, i.e. the
    bytes a dense upload would have put there (maskUtils.decode in get_isegmap, coco_ds.py:265-278, moved behind the
    bus).  One upload of the run ends and records, one launch; only the runs cross the bus.  ``out``: a contiguous uint8
    tensor of that shape to write; else a fresh one on ``device`` (default: the current GPU).  An entry without masks
    launches nothing."""
    n, (wy, wx, wh, ww), out = _masks_front(m, window, out, device, 'rle_decode_masks')
    if n == 0:
        return out
    first = np.asarray(m.first, np.int64)
    recs = np.empty((n, RLE_REC_INTS), np.int32)
    recs[:, :6] = (m.shape[1], m.shape[2], wy, wx, wh, ww)
    recs[:, 6] = first[:-1]
    recs[:, 7] = np.diff(first)
    _rle_decode([m.ends], recs, out, wh * ww, wh, ww)
    return out


def rle_decode_rows(slot: torch.Tensor, items: list) -> torch.Tensor:
    """``rle_decode_masks`` into rows of an existing slot (the support path: ``spp_msk``, the static slot of a captured
    graph included): ``slot`` uint8 [rows, capacity], contiguous; ``items`` = (row, RleMasks of ONE mask, window) each:
    the window's wh * ww bytes go to the front of that row, what lies behind them and every other row stays as it is.
    One upload, one launch for all items; none, no launch."""
    items = _row_items(slot, items, 'rle_decode_rows')
    if not items:
        return slot
    rows, cap = slot.shape
    recs = np.zeros((rows, RLE_REC_INTS), np.int32)          # (an all-zero record has an empty window: nothing is written)
    parts, run0 = [], 0
    for row, m, window in items:
        recs[row] = (m.shape[1], m.shape[2]) + window + (run0, m.ends.size)
        parts.append(m.ends)
        run0 += int(m.ends.size)
    _rle_decode(parts, recs, slot, cap, max(w[2] for _, _, w in items), max(w[3] for _, _, w in items))
    return slot


CM_REC_INTS = 16             # csrc/mask.hip: {row, h, w, y0, x0, y1, x1, lo[3], hi[3], out, 0, 0} per mask


def _color_records(items: list, rows: int, cap: int, fn: str) -> list:
    """``items`` = (row, ``colormask.ColorMasks``) each, checked against a [rows, cap] image slot -> per item the
    int32 records [n_i, 16] with the output index still 0."""
    recs = []
    for row, m in items:
        n, h, w = m.shape
        if not 0 <= int(row) < rows:
            raise _lib.FgnHipError(f'{fn}: row {row} is outside the {rows} rows of the image slot')
        if not (1 <= h <= RESIZE_MAX_DIM and 1 <= w <= RESIZE_MAX_DIM) or 3 * h * w > cap:
            raise _lib.FgnHipError(f'{fn}: an image of {h}x{w} pixels does not fit a slot row of {cap} bytes')
        r = np.zeros((n, CM_REC_INTS), np.int32)
        r[:, 0], r[:, 1], r[:, 2] = int(row), h, w
        r[:, 3:7] = m.boxes
        r[:, 7:10], r[:, 10:13] = m.bounds()
        recs.append(r)
    return recs


def _color_launch(src_slot: torch.Tensor, recs: np.ndarray, out: torch.Tensor, out_stride: int, n_out: int, max_h: int,
                  max_w: int) -> None:
    """ONE upload of the records and ONE launch of ``fgn_color_mask_u8``, on the current stream - behind whatever that
    stream has queued, the copy of the image bytes into ``src_slot`` included."""
    rows, cap = src_slot.shape
    dev_recs = torch.from_numpy(np.ascontiguousarray(recs, np.int32)).to(out.device, non_blocking=True)
    _lib.check(_lib.load().fgn_color_mask_u8(_ptr(src_slot), int(src_slot.stride(0)) if rows > 1 else int(cap), int(cap),
                                             int(rows), _ptr(dev_recs), int(recs.shape[0]), _ptr(out), int(out_stride),
                                             int(n_out), int(max_h), int(max_w), _stream()), 'fgn_color_mask_u8')


def _image_slot(src_slot: torch.Tensor, fn: str) -> None:
    if not src_slot.is_cuda or src_slot.dtype != torch.uint8 or src_slot.dim() != 2:
        raise _lib.FgnHipError(f'{fn}: src_slot must be a uint8 device tensor [rows, capacity]')
    if (src_slot.shape[1] > 1 and src_slot.stride(1) != 1) or (src_slot.shape[0] > 1 and
                                                               src_slot.stride(0) < src_slot.shape[1]):
        raise _lib.FgnHipError(f'{fn}: the rows of src_slot must be dense and must not overlap (a view of rows at any '
                               f'byte offset and pitch is fine)')


def color_masks(src_slot: torch.Tensor, items: list, out: Optional[torch.Tensor] = None) -> list:
    """Masks from box + colour (``colormask.ColorMasks``; get_char_mask_by_color, create_img_from_chars.py:136-158,
    moved behind the bus): ``src_slot`` uint8 [rows, capacity] on the device, row r holding an image [h,w,3] at its
    front (``qry_src``, or a [B,H,W,3] batch viewed as [B, H*W*3]; rows may start at any byte); ``items`` = (row,
    ColorMasks at that image's size) each.  -> per item the dense masks uint8 0/1 [n_i,h_i,w_i]:
    ``ColorMasks.dense`` bit for bit, written in full.  One upload of the records (16 ints per mask), one launch for all
    items, on the current stream - which must be the one that carries the copy of the image bytes, or wait for it.
    ``out``: a contiguous uint8 [total masks, max h*w] to write; else a fresh one.  The items' masks are views of it
    (copies for an image smaller than the largest).  No mask at all: no launch."""
    _image_slot(src_slot, 'color_masks')
    rows, cap = src_slot.shape
    recs = _color_records(items, rows, cap, 'color_masks')
    total = int(sum(r.shape[0] for r in recs))
    stride = max((m.shape[1] * m.shape[2] for _, m in items if m.shape[0]), default=0)
    if out is None:
        out = torch.empty((total, stride), device=src_slot.device, dtype=torch.uint8)
    else:
        _chk(out, 'out', torch.uint8)
        if tuple(out.shape) != (total, stride):
            raise _lib.FgnHipError(f'color_masks: out is {tuple(out.shape)}, expected {(total, stride)}')
    if total:
        allr = np.concatenate(recs)
        allr[:, 13] = np.arange(total)
        _color_launch(src_slot, allr, out, stride, total, max(m.shape[1] for _, m in items if m.shape[0]),
                      max(m.shape[2] for _, m in items if m.shape[0]))
    res, first = [], 0
    for _, m in items:
        n, h, w = m.shape
        res.append(out[first:first + n, :h * w].reshape(n, h, w) if n else
                   torch.zeros((0, h, w), device=src_slot.device, dtype=torch.uint8))
        first += n
    return res


def color_mask_rows(src_slot: torch.Tensor, msk_slot: torch.Tensor, items: list) -> torch.Tensor:
    """``color_masks`` for the support path: ``src_slot`` uint8 [rows, capacity] holds instance i's image window
    [wh,ww,3] at the front of row i (``spp_src``), ``msk_slot`` uint8 [rows, mask capacity], contiguous (``spp_msk``, the
    static slot of a captured graph included); ``items`` = (row, ColorMasks of ONE mask at the window's size, its box in
    the window's frame) each: the mask's wh * ww bytes go to the front of that row of ``msk_slot`` - the layout
    ``rle_decode_rows`` writes -, what lies behind them and every other row stays as it is.  One upload, one launch for
    all items, on the current stream; none, no launch."""
    _image_slot(src_slot, 'color_mask_rows')
    _chk(msk_slot, 'msk_slot', torch.uint8)
    if msk_slot.dim() != 2 or msk_slot.shape[0] != src_slot.shape[0]:
        raise _lib.FgnHipError('color_mask_rows: msk_slot must be [rows, capacity] with the rows of src_slot')
    if not items:
        return msk_slot
    rows, mcap = msk_slot.shape
    seen = set()
    for row, m in items:
        if m.shape[0] != 1 or int(row) in seen:
            raise _lib.FgnHipError(f'color_mask_rows: row {row}: one mask per item, one item per row')
        seen.add(int(row))
        if m.shape[1] * m.shape[2] > mcap:
            raise _lib.FgnHipError(f'color_mask_rows: a window of {m.shape[1] * m.shape[2]} bytes exceeds the slot '
                                   f'capacity {mcap}')
    recs = np.concatenate(_color_records(items, rows, src_slot.shape[1], 'color_mask_rows'))
    recs[:, 13] = recs[:, 0]
    _color_launch(src_slot, recs, msk_slot, mcap, rows, max(m.shape[1] for _, m in items),
                  max(m.shape[2] for _, m in items))
    return msk_slot


POLY_REC_INTS = 8            # csrc/poly.hip: mask {h, w, wy, wx, wh, ww, part0, n_parts}, part {edge0, n_edges, points,
#                              ends0, cap, h, w, 0}, edge {xs, ys, steps, major | flip << 1, s lo, s hi, first, 0}


def _poly_launch(entries: list, n_out: int, out: torch.Tensor, stride: int, max_wh: int, max_ww: int) -> int:
    """ONE upload - [mask records | part records | edge records], int32, 8 per record - and ONE call of
    ``fgn_poly_masks_u8`` (two launches) into ``out`` (output i at byte i * stride), on the current stream.  ``entries``
    = (output index, (h, w), (wy, wx, wh, ww), the instance's parts) each; an output without an entry keeps an all-zero
    record, whose empty window writes nothing.  -> the bytes uploaded."""
    from . import polygon
    recs = np.zeros((n_out, POLY_REC_INTS), np.int32)
    parts, edges, n_edges, ends0 = [], [], 0, 0
    for i, (h, w), window, inst in entries:
        recs[i] = (h, w) + tuple(window) + (len(parts), len(inst))
        for xy in inst:
            e, points, cap = polygon.edge_records(xy)
            if cap > polygon.CROSSING_CAP or points > polygon.POINT_CAP:
                raise _lib.FgnHipError(f'poly_masks: a part of {points} points / up to {cap} crossings exceeds what the '
                                       f'device takes; such an instance goes the host route')
            parts.append((n_edges, len(e), points, ends0, cap, h, w, 0))
            edges.append(e)
            n_edges += len(e)
            ends0 += cap
    tables = [recs.reshape(-1), np.asarray(parts, np.int32).reshape(-1)] + [e.reshape(-1) for e in edges]
    blob = torch.from_numpy(np.concatenate(tables).astype(np.int32, copy=False)).to(out.device, non_blocking=True)
    scratch = torch.empty(max(ends0, 1), device=out.device, dtype=torch.int32)
    _lib.check(_lib.load().fgn_poly_masks_u8(_ptr(blob), int(blob.numel()), int(n_out), len(parts), int(n_edges),
                                             _ptr(scratch), int(scratch.numel()), _ptr(out), int(stride), int(max_wh),
                                             int(max_ww), _stream()), 'fgn_poly_masks_u8')
    return int(blob.numel()) * 4


def poly_masks(pm, window=None, out: Optional[torch.Tensor] = None, device=None,
               routes: Optional[list] = None) -> torch.Tensor:
    """The n masks of a ``polygon.PolyMasks`` (what ``polygon.as_polys`` makes of COCO polygons) -> dense uint8 0/1
    [n,h,w] on the device, or [n,wh,ww] for one ``window`` = (wy, wx, wh, ww) of every mask: ``polygon.dense`` bit for
    bit, i.e. the bytes a dense upload would have put there (maskUtils.frPyObjects + merge + decode, moved behind the
    bus).  One upload of the records, two launches (crossings, fill); only vertices cross the bus.  The route is decided
    on the host before anything is queued (``PolyMasks.on_host``): an instance with a part over the device's capacity
    travels as ``polygon.to_rle`` through ``rle_decode_masks`` instead.  ``routes``: a list that receives 'device' or
    'host' per instance.  ``out``: a contiguous uint8 tensor of that shape to write; else a fresh one on ``device``
    (default: the current GPU).  An entry without masks launches nothing."""
    from . import rle
    n, (wy, wx, wh, ww), out = _masks_front(pm, window, out, device, 'poly_masks')
    host = pm.on_host()
    if routes is not None:
        routes.extend('host' if v else 'device' for v in host)
    if n == 0:
        return out
    hw = (int(pm.shape[1]), int(pm.shape[2]))
    entries = [(i, hw, (wy, wx, wh, ww), pm.parts(i)) for i in range(n) if not host[i]]
    if entries:
        _poly_launch(entries, n, out, wh * ww, wh, ww)
    idx = np.flatnonzero(host)
    if idx.size:
        runs = rle.as_masks(pm.rle_items(idx), hw, 'poly_masks')
        if idx.size == n:
            rle_decode_masks(runs, window, out=out)
        else:
            out[torch.from_numpy(idx).to(out.device)] = rle_decode_masks(runs, window, device=out.device)
    return out


def poly_mask_rows(slot: torch.Tensor, items: list, routes: Optional[list] = None) -> torch.Tensor:
    """``poly_masks`` into rows of an existing slot (the support path: ``spp_msk``, the static slot of a captured graph
    included): ``slot`` uint8 [rows, capacity], contiguous; ``items`` = (row, PolyMasks of ONE mask, window) each: the
    window's wh * ww bytes go to the front of that row - the layout ``rle_decode_rows`` writes -, what lies behind them
    and every other row stays as it is.  One upload, two launches for all items of the device route; those of the host
    route go through ``rle_decode_rows``; none, no launch.  ``routes`` as for ``poly_masks``, per item."""
    from . import rle
    items = _row_items(slot, items, 'poly_mask_rows')
    if not items:
        return slot
    rows, cap = slot.shape
    entries, on_host, max_wh, max_ww = [], [], 0, 0
    for row, m, window in items:
        hw = (int(m.shape[1]), int(m.shape[2]))
        host = bool(m.on_host()[0])
        if routes is not None:
            routes.append('host' if host else 'device')
        if host:
            on_host.append((row, rle.as_masks(m.rle_items([0]), hw, 'poly_mask_rows'), window))
        else:
            entries.append((row, hw, window, m.parts(0)))
            max_wh, max_ww = max(max_wh, window[2]), max(max_ww, window[3])
    if entries:
        _poly_launch(entries, rows, slot, cap, max_wh, max_ww)
    rle_decode_rows(slot, on_host)
    return slot


def mask_bits(masks: torch.Tensor):
    """Bit planes of dense binary masks [G,H,W] (bool / uint8, non-zero = set), the ground-truth operand of
    ``mask_overlap``: returns (bits int64 [H, ceil(W/64), G] - bit b of word xw of a row = pixel 64 xw + b - ,
    area [G] int32, (H, W))."""
    if masks.dtype == torch.bool:
        masks = masks.view(torch.uint8)
    _chk(masks, 'masks', torch.uint8)
    if masks.dim() != 3:
        raise _lib.FgnHipError('mask_bits: masks must be [G,H,W]')
    g, h, w = masks.shape
    bits = torch.empty((h, (w + 63) // 64, g), device=masks.device, dtype=torch.int64)
    area = torch.empty((g,), device=masks.device, dtype=torch.int32)
    _lib.check(_lib.load().fgn_mask_bits_u64(_ptr(masks), _ptr(bits), _ptr(area), g, h, w, _stream()),
               'fgn_mask_bits_u64')
    return bits, area, (h, w)


def mask_overlap(prob: torch.Tensor, boxes: torch.Tensor, gt_masks, img_h: int, img_w: int, thr: float,
                 n_dev: Optional[torch.Tensor] = None, skip_empty: bool = True, packed: bool = False):
    """Exact overlap counts of the pasted, thresholded detection masks (``prob`` [D,M,M], ``boxes`` [D,>=4], ``thr``,
    ``n_dev``, ``skip_empty`` as for ``mask_rle`` / ``mask_paste``: the same bits, never written) with the ground-truth
    masks ``gt_masks`` ([G,H,W] bool / uint8, or what ``mask_bits`` returned for them).  Returns (inter [D,G] int32 =
    |d & g|, det_area [D] int32 = |d|, gt_area [G] int32 = |g|), the three being views of ONE int32 allocation laid out
    [inter | det_area | gt_area]; ``packed``: that allocation is returned as a fourth value (one device-to-host copy
    moves them all).  Rows at or beyond the device count are zero.  With G == 0 nothing is launched and det_area is
    zero."""
    _chk(prob, 'prob')
    _chk(boxes, 'boxes')
    d, m, _ = prob.shape
    if boxes.shape[0] != d or boxes.shape[1] < 4:
        raise _lib.FgnHipError('mask_overlap: boxes shape mismatch')
    if n_dev is not None:
        _chk(n_dev, 'n_dev', torch.int32)
    bits, gt_area, hw = gt_masks if isinstance(gt_masks, tuple) else mask_bits(gt_masks)
    if tuple(hw) != (img_h, img_w):
        raise _lib.FgnHipError(f'mask_overlap: ground-truth masks are {tuple(hw)}, image is {(img_h, img_w)}')
    g = gt_area.numel()
    buf = torch.empty(d * g + d + g, device=prob.device, dtype=torch.int32)
    inter, det_area, ga = buf[:d * g].view(d, g), buf[d * g:d * g + d], buf[d * g + d:]
    if g:
        ga.copy_(gt_area)
    if d == 0 or g == 0:
        det_area.zero_()
        return (inter, det_area, ga, buf) if packed else (inter, det_area, ga)
    rc = _lib.load().fgn_mask_overlap_i32(_ptr(prob), _ptr(boxes), boxes.shape[1], _ptr(bits), _ptr(inter),
                                          _ptr(det_area), _ptr(n_dev), d, g, img_h, img_w, m, float(thr),
                                          int(bool(skip_empty)), _stream())
    _lib.check(rc, 'fgn_mask_overlap_i32')
    return (inter, det_area, ga, buf) if packed else (inter, det_area, ga)


def mask_overlap_src(prob: torch.Tensor, boxes: torch.Tensor, gt_masks, src_hw, net_hw, thr: float,
                     n_dev: Optional[torch.Tensor] = None, skip_empty: bool = True, packed: bool = False):
    """``mask_overlap`` of one image with the detections pasted at SOURCE size: ``boxes`` are in the frame of the
    ``net_hw`` = (H, W) network and are divided by the scale of the ``src_hw`` = (h, w) image as ``mask_rle_src`` divides
    them; ``gt_masks`` ([G,h,w] bool / uint8, or what ``mask_bits`` returned for them) are at source size as given.
    Returns what ``mask_overlap`` returns."""
    _chk(prob, 'prob')
    _chk(boxes, 'boxes')
    d, m, _ = prob.shape
    if boxes.shape[0] != d or boxes.shape[1] < 4:
        raise _lib.FgnHipError('mask_overlap_src: boxes shape mismatch')
    if n_dev is not None:
        _chk(n_dev, 'n_dev', torch.int32)
    h, w = int(src_hw[0]), int(src_hw[1])
    H, W = int(net_hw[0]), int(net_hw[1])
    if not all(1 <= v <= RESIZE_MAX_DIM for v in (h, w, H, W)):
        raise _lib.FgnHipError(f'mask_overlap_src: sizes must be within 1..{RESIZE_MAX_DIM}, got {(h, w)} and {(H, W)}')
    bits, gt_area, hw = gt_masks if isinstance(gt_masks, tuple) else mask_bits(gt_masks)
    if tuple(hw) != (h, w):
        raise _lib.FgnHipError(f'mask_overlap_src: ground-truth masks are {tuple(hw)}, the source image is {(h, w)}')
    g = gt_area.numel()
    buf = torch.empty(d * g + d + g, device=prob.device, dtype=torch.int32)
    inter, det_area, ga = buf[:d * g].view(d, g), buf[d * g:d * g + d], buf[d * g + d:]
    if g:
        ga.copy_(gt_area)
    if d == 0 or g == 0:
        det_area.zero_()
        return (inter, det_area, ga, buf) if packed else (inter, det_area, ga)
    rc = _lib.load().fgn_mask_overlap_src_i32(_ptr(prob), _ptr(boxes), boxes.shape[1], _ptr(bits), _ptr(inter),
                                              _ptr(det_area), _ptr(n_dev), d, g, h, w, H, W, m, float(thr),
                                              int(bool(skip_empty)), _stream())
    _lib.check(rc, 'fgn_mask_overlap_src_i32')
    return (inter, det_area, ga, buf) if packed else (inter, det_area, ga)


EVAL_MAX_THRS = 16


def eval_match(boxes: torch.Tensor, labels: torch.Tensor, gt_xywh, gt_cat, iou_thrs, n_ways: int, overlap=None,
               n_dev: Optional[torch.Tensor] = None, max_dets: int = 100, src_hw=None, net_hw=None,
               packed: bool = False):
    """The evaluator's greedy matching of one image on the device (``fsiseg_eval.match_flags`` bit for bit):
    ``boxes`` [D,>=5] (x1, y1, x2, y2, score) and ``labels`` [D] int64 as ``detect_device`` holds them, ``n_dev`` the
    device-side count; ``gt_xywh`` [G,4] float64 = ``fsiseg_eval._xywh(qry_bboxes)`` and ``gt_cat`` [G] (host arrays are
    uploaded: G is small); ``iou_thrs``: 1..16 thresholds as the evaluator is given them (the cap at 1 - 1e-10 is applied
    here); ``overlap``: (inter [D,G], det_area [D], gt_area [G]) of ``mask_overlap`` / ``mask_overlap_src``, or None =
    no segm flags.  ``src_hw`` / ``net_hw``: the boxes are network-frame boxes to be divided by the image's scale
    (``results_at_source``), as ``mask_overlap_src`` divides them.  Returns (bbox flags [D], segm flags [D] or None),
    int32 views of ONE allocation [2, D]; ``packed``: that allocation as a third value.  Bit t = matched at
    ``iou_thrs[t]``, -1 = beyond ``max_dets`` of its category, 0 = label outside 0..n_ways-1 or row at / beyond the
    device count."""
    _chk(boxes, 'boxes')
    _chk(labels, 'labels', torch.int64)
    d = boxes.shape[0]
    if boxes.dim() != 2 or boxes.shape[1] < 5 or labels.shape != (d,):
        raise _lib.FgnHipError('eval_match: boxes must be [D,>=5] and labels [D]')
    if n_dev is not None:
        _chk(n_dev, 'n_dev', torch.int32)
    dev = boxes.device
    thrs = np.minimum(np.asarray(iou_thrs, np.float64).reshape(-1), 1 - 1e-10)
    xywh = gt_xywh.detach().cpu().numpy() if isinstance(gt_xywh, torch.Tensor) else np.asarray(gt_xywh)
    xywh = np.ascontiguousarray(xywh, np.float64).reshape(-1, 4)
    cat = gt_cat.detach().cpu().numpy() if isinstance(gt_cat, torch.Tensor) else np.asarray(gt_cat)
    cat = np.ascontiguousarray(cat.reshape(-1), np.int32)
    g = xywh.shape[0]
    if cat.shape[0] != g:
        raise _lib.FgnHipError(f'eval_match: {g} ground-truth boxes, {cat.shape[0]} categories')
    inter = det_area = gt_area = None
    if overlap is not None:
        inter, det_area, gt_area = overlap[:3]
        for t, name, shape in ((inter, 'inter', (d, g)), (det_area, 'det_area', (d,)), (gt_area, 'gt_area', (g,))):
            _chk(t, name, torch.int32)
            if tuple(t.shape) != shape:
                raise _lib.FgnHipError(f'eval_match: {name} is {tuple(t.shape)}, expected {shape}')
    buf = torch.empty((2, d), device=dev, dtype=torch.int32)
    out = (buf[0], buf[1] if overlap is not None else None)
    if d == 0:
        return out + (buf,) if packed else out
    # ONE upload for the host operands: [thr float64 [T] | gt_xywh float64 [G,4] | gt_cat int32 [G]] as bytes
    t_n = thrs.shape[0]
    blob = torch.from_numpy(np.concatenate([thrs.view(np.uint8), xywh.reshape(-1).view(np.uint8),
                                            cat.view(np.uint8)])).to(dev, non_blocking=True)
    base = blob.data_ptr()
    sh, sw = (int(src_hw[0]), int(src_hw[1])) if src_hw is not None else (0, 0)
    nh, nw = (int(net_hw[0]), int(net_hw[1])) if net_hw is not None else (0, 0)
    if src_hw is not None and net_hw is None:
        raise _lib.FgnHipError('eval_match: src_hw needs net_hw')
    rc = _lib.load().fgn_eval_match_i32(_ptr(boxes), boxes.shape[1], _ptr(labels), _ptr(n_dev), _ptr(inter),
                                        _ptr(det_area), _ptr(gt_area), base + 8 * t_n if g else None,
                                        base + 8 * t_n + 32 * g if g else None, base, _ptr(buf), d, g, t_n, int(n_ways),
                                        int(max_dets), sh, sw, nh, nw, _stream())
    _lib.check(rc, 'fgn_eval_match_i32')
    return out + (buf,) if packed else out


# --------------------------------------------------------------------------------------
# forward_train pieces (csrc/train.hip)
# --------------------------------------------------------------------------------------
def box_assign(boxes: torch.Tensor, gts: torch.Tensor, pos_iou_thr: float, neg_iou_thr: float, min_pos_iou: float,
               match_low_quality: bool = True, inside: Optional[torch.Tensor] = None, with_overlaps: bool = False,
               out: Optional[torch.Tensor] = None):
    """MaxIoUAssigner: boxes [n, >=4], gts [k,4] -> gt_inds [n] int32 (-2 not a candidate, -1 ignored, 0 negative,
    i+1 positive of GT i) (+ max_overlaps [n]).  ``out``: an int32 [n] slice to write into."""
    _chk(boxes, 'boxes')
    n, k = boxes.shape[0], gts.shape[0]
    if k:
        _chk(gts, 'gts')
    if inside is not None:
        _chk(inside, 'inside', torch.uint8)
    L = _lib.load()
    if out is None:
        gt_inds = torch.empty((n,), device=boxes.device, dtype=torch.int32)
    else:
        _chk(out, 'out', torch.int32)
        if out.numel() != n:
            raise _lib.FgnHipError('box_assign: out must hold n entries')
        gt_inds = out
    mo = torch.zeros((n,), device=boxes.device, dtype=torch.float32) if with_overlaps else None
    scratch = torch.empty(L.fgn_box_assign_scratch_bytes(n, k), device=boxes.device, dtype=torch.uint8)
    rc = L.fgn_box_assign_f32(_ptr(boxes), boxes.shape[1], _ptr(inside), _ptr(gts) if k else None, n, k,
                              float(pos_iou_thr), float(neg_iou_thr), float(min_pos_iou), int(match_low_quality),
                              _ptr(scratch), _ptr(gt_inds), _ptr(mo), _stream())
    _lib.check(rc, 'fgn_box_assign_f32')
    return (gt_inds, mo) if with_overlaps else gt_inds


def bbox2delta(proposals: torch.Tensor, gts: torch.Tensor, means, stds) -> torch.Tensor:
    _chk(proposals, 'proposals')
    _chk(gts, 'gts')
    n = proposals.shape[0]
    if tuple(proposals.shape) != (n, 4) or tuple(gts.shape) != (n, 4):
        raise _lib.FgnHipError('bbox2delta: operands must be [n,4]')
    out = torch.empty((n, 4), device=proposals.device, dtype=torch.float32)
    rc = _lib.load().fgn_bbox2delta_f32(_ptr(proposals), _ptr(gts), _ptr(out), n, _f4(means), _f4(stds), _stream())
    _lib.check(rc, 'fgn_bbox2delta_f32')
    return out


def _loss_args(x, y, w):
    _chk(x, 'pred')
    _chk(y, 'target')
    if x.numel() != y.numel():
        raise _lib.FgnHipError('loss: pred / target sizes differ')
    if w is not None:
        _chk(w, 'weight')
        if w.numel() != x.numel():
            raise _lib.FgnHipError('loss: weight size differs')


def bce_logits_sum(x, y, w, avg_factor: float, y_threshold: float = -1.0) -> torch.Tensor:
    """sum_i w_i * BCEWithLogits(x_i, y_i) / avg_factor -> [1] (y binarised at y_threshold when >= 0)."""
    _loss_args(x, y, w)
    out = torch.empty((1,), device=x.device, dtype=torch.float32)
    rc = _lib.load().fgn_bce_logits_sum_f32(_ptr(x), _ptr(y), _ptr(w), x.numel(), float(y_threshold),
                                            float(avg_factor), _ptr(out), _stream())
    _lib.check(rc, 'fgn_bce_logits_sum_f32')
    return out


def smooth_l1_sum(pred, target, w, avg_factor: float, beta: float = 1.0) -> torch.Tensor:
    _loss_args(pred, target, w)
    out = torch.empty((1,), device=pred.device, dtype=torch.float32)
    rc = _lib.load().fgn_smooth_l1_sum_f32(_ptr(pred), _ptr(target), _ptr(w), pred.numel(), float(beta),
                                           float(avg_factor), _ptr(out), _stream())
    _lib.check(rc, 'fgn_smooth_l1_sum_f32')
    return out


def softmax_ce_sum(logits, labels, w, avg_factor: float) -> torch.Tensor:
    _chk(logits, 'logits')
    _chk(labels, 'labels', torch.int64)
    n, c = logits.shape
    if labels.numel() != n or (w is not None and w.numel() != n):
        raise _lib.FgnHipError('softmax_ce_sum: operand sizes differ')
    if w is not None:
        _chk(w, 'weight')
    out = torch.empty((1,), device=logits.device, dtype=torch.float32)
    rc = _lib.load().fgn_softmax_ce_sum_f32(_ptr(logits), _ptr(labels), _ptr(w), n, c, float(avg_factor), _ptr(out),
                                            _stream())
    _lib.check(rc, 'fgn_softmax_ce_sum_f32')
    return out


def bn_train(x: torch.Tensor, gamma, beta, eps: float, momentum: float, running_mean=None, running_var=None,
             residual=None, relu: bool = False, inplace: bool = True):
    """BatchNorm2d in training mode on NHWC x [..., C]: -> (y, batch mean [C], biased batch variance [C]); the
    running estimates (optional) are updated in place."""
    _chk(x, 'x')
    c = x.shape[-1]
    p = x.numel() // c
    for t, nm in ((gamma, 'gamma'), (beta, 'beta'), (running_mean, 'running_mean'), (running_var, 'running_var'),
                  (residual, 'residual')):
        if t is not None:
            _chk(t, nm)
    if residual is not None and residual.numel() != x.numel():
        raise _lib.FgnHipError('bn_train: residual shape differs')
    L = _lib.load()
    mean = torch.empty((c,), device=x.device, dtype=torch.float32)
    var = torch.empty((c,), device=x.device, dtype=torch.float32)
    out = x if inplace else torch.empty_like(x)
    scratch = torch.empty(L.fgn_bn_train_scratch_bytes(c), device=x.device, dtype=torch.uint8)
    rc = L.fgn_bn_train_f32(_ptr(x), p, c, _ptr(gamma), _ptr(beta), float(eps), float(momentum), _ptr(running_mean),
                            _ptr(running_var), _ptr(residual), int(relu), _ptr(scratch), _ptr(mean), _ptr(var),
                            _ptr(out), _stream())
    _lib.check(rc, 'fgn_bn_train_f32')
    return out, mean, var


# --------------------------------------------------------------------------------------
# backward pieces of the trainable heads (csrc/train_bwd.hip)
# --------------------------------------------------------------------------------------
def bce_logits_grad(x, y, w, scale: float, y_threshold: float = -1.0) -> torch.Tensor:
    _loss_args(x, y, w)
    dx = torch.empty_like(x)
    rc = _lib.load().fgn_bce_logits_grad_f32(_ptr(x), _ptr(y), _ptr(w), x.numel(), float(y_threshold), float(scale),
                                             _ptr(dx), _stream())
    _lib.check(rc, 'fgn_bce_logits_grad_f32')
    return dx


def smooth_l1_grad(pred, target, w, scale: float, beta: float = 1.0) -> torch.Tensor:
    _loss_args(pred, target, w)
    d = torch.empty_like(pred)
    rc = _lib.load().fgn_smooth_l1_grad_f32(_ptr(pred), _ptr(target), _ptr(w), pred.numel(), float(beta), float(scale),
                                            _ptr(d), _stream())
    _lib.check(rc, 'fgn_smooth_l1_grad_f32')
    return d


def softmax_ce_grad(logits, labels, w, scale: float) -> torch.Tensor:
    _chk(logits, 'logits')
    _chk(labels, 'labels', torch.int64)
    if w is not None:
        _chk(w, 'weight')
    n, c = logits.shape
    d = torch.empty_like(logits)
    rc = _lib.load().fgn_softmax_ce_grad_f32(_ptr(logits), _ptr(labels), _ptr(w), n, c, float(scale), _ptr(d), _stream())
    _lib.check(rc, 'fgn_softmax_ce_grad_f32')
    return d


def relu_backward(dy: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """dy * [y > 0] (y: the ReLU's output)."""
    _chk(dy, 'dy')
    _chk(y, 'y')
    if dy.numel() != y.numel():
        raise _lib.FgnHipError('relu_backward: operand sizes differ')
    out = torch.empty_like(dy)
    rc = _lib.load().fgn_relu_backward_f32(_ptr(dy), _ptr(y), _ptr(out), dy.numel(), _stream())
    _lib.check(rc, 'fgn_relu_backward_f32')
    return out


def colsum(x: torch.Tensor, out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """x [..., C] -> [C] = sum over all leading dims (fp64 partials, fixed order)."""
    _chk(x, 'x')
    c = x.shape[-1]
    r = x.numel() // c if c else 0
    L = _lib.load()
    if out is None:
        out = torch.empty((c,), device=x.device, dtype=torch.float32)
        accumulate = False
    else:
        _chk(out, 'out')
    scratch = torch.empty(L.fgn_colsum_scratch_bytes(c), device=x.device, dtype=torch.uint8)
    rc = L.fgn_colsum_f32(_ptr(x), r, c, _ptr(scratch), _ptr(out), int(accumulate), _stream())
    _lib.check(rc, 'fgn_colsum_f32')
    return out


def bn_train_backward(x_pre, y_post, dy, mean, var, gamma, eps: float, want_g: bool = False):
    """-> dx, dgamma, dbeta (+ g = dy masked by the ReLU, when ``want_g``)."""
    for t, nm in ((x_pre, 'x_pre'), (dy, 'dy'), (mean, 'mean'), (var, 'var'), (gamma, 'gamma')):
        _chk(t, nm)
    if y_post is not None:
        _chk(y_post, 'y_post')
    c = x_pre.shape[-1]
    p = x_pre.numel() // c
    if dy.numel() != x_pre.numel() or (y_post is not None and y_post.numel() != x_pre.numel()):
        raise _lib.FgnHipError('bn_train_backward: operand sizes differ')
    L = _lib.load()
    dx = torch.empty_like(x_pre)
    g = torch.empty_like(x_pre) if want_g else None
    dgamma = torch.empty((c,), device=x_pre.device, dtype=torch.float32)
    dbeta = torch.empty((c,), device=x_pre.device, dtype=torch.float32)
    scratch = torch.empty(L.fgn_bn_train_backward_scratch_bytes(c), device=x_pre.device, dtype=torch.uint8)
    rc = L.fgn_bn_train_backward_f32(_ptr(x_pre), _ptr(y_post), _ptr(dy), _ptr(mean), _ptr(var), _ptr(gamma), float(eps),
                                     p, c, _ptr(scratch), _ptr(dx), _ptr(g), _ptr(dgamma), _ptr(dbeta), _stream())
    _lib.check(rc, 'fgn_bn_train_backward_f32')
    return (dx, dgamma, dbeta, g) if want_g else (dx, dgamma, dbeta)


def relation_gn_head_backward(q, s, rois, gn_w, gn_b, fc_w, d_out6, n_ways: int, gn_groups: int, eps: float):
    """-> dQ [R,7,7,C], dZ [R*N,7,7,C], pooled [R*N,C], dgamma [C], dbeta [C]."""
    for t, nm in ((q, 'Q'), (s, 'S'), (rois, 'rois'), (gn_w, 'gn_w'), (gn_b, 'gn_b'), (fc_w, 'fc_w'), (d_out6, 'd_out6')):
        _chk(t, nm)
    r, ps, _, c = q.shape
    if tuple(d_out6.shape) != (r * n_ways, 6) or tuple(fc_w.shape) != (6, c):
        raise _lib.FgnHipError('relation_gn_head_backward: operand shapes inconsistent')
    dq = torch.empty_like(q)
    dz = torch.empty((r * n_ways, ps, ps, c), device=q.device, dtype=torch.float32)
    pooled = torch.empty((r * n_ways, c), device=q.device, dtype=torch.float32)
    dga = torch.empty((r, c), device=q.device, dtype=torch.float32)
    dbe = torch.empty((r, c), device=q.device, dtype=torch.float32)
    rc = _lib.load().fgn_relation_gn_head_backward_f32(_ptr(q), _ptr(s), _ptr(rois), _ptr(gn_w), _ptr(gn_b), _ptr(fc_w),
                                                       _ptr(d_out6), _ptr(dq), _ptr(dz), _ptr(pooled), _ptr(dga),
                                                       _ptr(dbe), r, n_ways, c, gn_groups, ps, float(eps), _stream())
    _lib.check(rc, 'fgn_relation_gn_head_backward_f32')
    return dq, dz, pooled, colsum(dga), colsum(dbe)


def mask_logits_backward(up: torch.Tensor, dlogit: torch.Tensor, w: torch.Tensor, roi_size: int):
    """up [D,P,P,4*C], dlogit [D,2P,2P], w [C] -> d_up [D,P,P,4*C], dw [C]."""
    _chk(up, 'up')
    _chk(dlogit, 'dlogit')
    _chk(w, 'w')
    d, c = up.shape[0], w.numel()
    if up.numel() != d * roi_size * roi_size * 4 * c or tuple(dlogit.shape) != (d, 2 * roi_size, 2 * roi_size):
        raise _lib.FgnHipError('mask_logits_backward: operand shapes inconsistent')
    d_up = torch.empty_like(up)
    part = torch.empty((d, c), device=up.device, dtype=torch.float32)
    rc = _lib.load().fgn_mask_logits_backward_f32(_ptr(up), _ptr(dlogit), _ptr(w), _ptr(d_up), _ptr(part), d, roi_size, c,
                                                  _stream())
    _lib.check(rc, 'fgn_mask_logits_backward_f32')
    return d_up, colsum(part)


def im2col3x3(x: torch.Tensor) -> torch.Tensor:
    """x [n,H,W,C] -> [n*H*W, 9*C] (3x3, stride 1, pad 1; column = tap*C + ci)."""
    _chk(x, 'x')
    n, h, w, c = x.shape
    out = torch.empty((n * h * w, 9 * c), device=x.device, dtype=torch.float32)
    rc = _lib.load().fgn_im2col3x3_f32(_ptr(x), _ptr(out), n, h, w, c, _stream())
    _lib.check(rc, 'fgn_im2col3x3_f32')
    return out


def gemm_tn(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a [R,M], b [R,N] -> a^T b [M,N] (the weight-gradient product: reduction over the rows) on the MFMA kernel."""
    _chk(a, 'a')
    _chk(b, 'b')
    r, m = a.shape
    n = b.shape[1]
    if b.shape[0] != r:
        raise _lib.FgnHipError('gemm_tn: operands must share the row count')
    L = _lib.load()
    out = torch.empty((m, n), device=a.device, dtype=torch.float32)
    wsb = L.fgn_gemm_tn_workspace_bytes(r, m, n)
    ws = torch.empty(wsb, device=a.device, dtype=torch.uint8) if wsb else None
    rc = L.fgn_gemm_tn_f32(_ptr(a), _ptr(b), _ptr(out), r, m, n, _ptr(ws), _stream())
    _lib.check(rc, 'fgn_gemm_tn_f32')
    return out


def gemm_small(a: torch.Tensor, b: torch.Tensor, trans_a: bool = False) -> torch.Tensor:
    """a [M,K] (or [K,M] with ``trans_a``) x b [K,N] -> [M,N] on the one-thread-per-output kernel: the products whose
    shapes the MFMA kernels do not take (a dimension that is not a multiple of 4 / 32).  Operands may be row-strided
    2-D views (unit stride along the last dimension)."""
    for t, nm in ((a, 'a'), (b, 'b')):
        if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
            raise _lib.FgnHipError(f'gemm_small: {nm} must be a 2-D fp32 device tensor with unit inner stride')
    k, m = (a.shape[0], a.shape[1]) if trans_a else (a.shape[1], a.shape[0])
    if b.shape[0] != k:
        raise _lib.FgnHipError('gemm_small: inner dimensions differ')
    n = b.shape[1]
    out = torch.empty((m, n), device=a.device, dtype=torch.float32)
    lda = a.stride(0) if a.shape[0] > 1 else a.shape[1]
    ldb = b.stride(0) if b.shape[0] > 1 else n
    rc = _lib.load().fgn_gemm_small_f32(_ptr(a), _ptr(b), _ptr(out), m, n, k, lda, ldb, n, int(trans_a), _stream())
    _lib.check(rc, 'fgn_gemm_small_f32')
    return out


def roi_align_backward(dy: torch.Tensor, rois: torch.Tensor, fmap_shape, spatial_scale: float, sampling_ratio: int,
                       aligned: bool, out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """The adjoint of ``roi_align`` (no post_shift, no ReLU): dy [R,P,P,C], rois [R,5] -> dx ``fmap_shape`` = [B,H,W,C].
    ``out`` with ``accumulate``: added onto; otherwise overwritten (R = 0: zeros).  Gather form without atomics: the
    terms of an element are added in (RoI index, bin row, bin column) order, so two runs give the same bytes."""
    _chk(dy, 'dy')
    _chk(rois, 'rois')
    b, h, w, c = (int(v) for v in fmap_shape)
    if rois.dim() != 2 or rois.shape[1] != 5:
        raise _lib.FgnHipError('roi_align_backward: rois must be [R,5]')
    r = rois.shape[0]
    if dy.dim() != 4 or dy.shape[0] != r or dy.shape[1] != dy.shape[2] or dy.shape[3] != c:
        raise _lib.FgnHipError('roi_align_backward: dy must be [R,P,P,C] for rois [R,5] and a [B,H,W,C] map')
    if out is None:
        out = torch.empty((b, h, w, c), device=dy.device, dtype=torch.float32)
        accumulate = False
    else:
        _chk(out, 'out')
        if tuple(out.shape) != (b, h, w, c):
            raise _lib.FgnHipError('roi_align_backward: bad out shape')
    rc = _lib.load().fgn_roi_align_backward_nhwc_f32(_ptr(dy), _ptr(rois), _ptr(out), r, b, h, w, c, int(dy.shape[1]),
                                                     float(spatial_scale), int(sampling_ratio), int(aligned),
                                                     int(accumulate), _stream())
    _lib.check(rc, 'fgn_roi_align_backward_nhwc_f32')
    return out


def guidance_index(g, y, x, batch: int, n_ways: int, h: int, w: int) -> dict:
    """The host-side index of ``guidance_backward``.  Active row r of the gradient in front of rpn_conv's ReLU sits at
    pixel (y[r], x[r]) of guided pass g[r] = b * n_ways + n; its tap ky*3+kx reaches the pixel (y + ky - 1, x + kx - 1)
    of image b (taps that fall outside the map are dropped).  -> dict of int32 arrays in CSR form: ``pix`` [touched]
    flat pixels b*h*w + y*w + x, ascending; ``seg`` [touched*n_ways + 1]: the entries of (touched pixel t, pass n) are
    ``ent[seg[t*n_ways+n] : seg[t*n_ways+n+1]]``; ``ent`` [nnz] = r*9 + tap, ascending within a segment; ``img_seg``
    [batch + 1]: the touched pixels of image b are ``pix[img_seg[b] : img_seg[b+1]]``."""
    g, y, x = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (g, y, x))
    if not (g.size == y.size == x.size):
        raise ValueError('guidance_index: g, y and x must have one entry per active row')
    if g.size and (g.min() < 0 or g.max() >= batch * n_ways or y.min() < 0 or y.max() >= h or x.min() < 0 or x.max() >= w):
        raise ValueError('guidance_index: a row lies outside the [batch*n_ways, h, w] map')
    tap = np.arange(9, dtype=np.int64)[None, :]
    ty, tx = y[:, None] + tap // 3 - 1, x[:, None] + tap % 3 - 1
    ok = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
    pixel = ((g[:, None] // n_ways) * h + ty) * w + tx
    key = pixel * n_ways + g[:, None] % n_ways                    # (pixel, pass)
    entry = np.arange(g.size, dtype=np.int64)[:, None] * 9 + tap
    key, entry = key[ok], entry[ok]
    order = np.lexsort((entry, key))
    key, entry = key[order], entry[order]
    pix = np.unique(key // n_ways)
    t = np.searchsorted(pix, key // n_ways)
    counts = np.bincount(t * n_ways + key % n_ways, minlength=pix.size * n_ways)
    seg = np.concatenate([[0], np.cumsum(counts)])
    img_seg = np.searchsorted(pix, np.arange(batch + 1, dtype=np.int64) * h * w)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    return dict(pix=i32(pix), seg=i32(seg), ent=i32(entry), img_seg=i32(img_seg))


def guidance_backward(taps: torch.Tensor, index: dict, qry_fmap: torch.Tensor, vec: torch.Tensor,
                      out: Optional[torch.Tensor] = None, accumulate: bool = False, upload=None):
    """Backward of the AG-RPN guidance ``qry_fmap[b] * vec[b*N+n]`` from the sparse gradient of rpn_conv's input:
    taps [rows,9,C] (tap ky*3+kx of active row r), ``index`` = ``guidance_index`` (host arrays; checked here against
    the operand shapes, then uploaded in one copy - ``upload``: host int32 array -> device tensor, default a plain
    copy), qry_fmap [B,h,w,C], vec [B*N,C] -> (d_qry [B,h,w,C], d_vec [B*N,C]).  ``out`` with ``accumulate``: d_qry is
    added onto it at the touched pixels and left as it was elsewhere; otherwise zero at untouched pixels."""
    _chk(taps, 'taps')
    _chk(qry_fmap, 'qry_fmap')
    _chk(vec, 'vec')
    b, h, w, c = qry_fmap.shape
    if vec.dim() != 2 or vec.shape[1] != c or vec.shape[0] % b:
        raise _lib.FgnHipError('guidance_backward: vec must be [B*N,C]')
    n = vec.shape[0] // b
    rows = taps.shape[0]
    if taps.dim() != 3 or taps.shape[1] != 9 or taps.shape[2] != c:
        raise _lib.FgnHipError('guidance_backward: taps must be [rows,9,C]')
    pix, seg, ent, img_seg = (np.ascontiguousarray(index[k], dtype=np.int32) for k in ('pix', 'seg', 'ent', 'img_seg'))
    nt = pix.size
    bad = seg.size != nt * n + 1 or img_seg.size != b + 1 or seg[0] != 0 or seg[-1] != ent.size \
        or (np.diff(seg) < 0).any() or (np.diff(img_seg) < 0).any() or img_seg[0] != 0 or img_seg[-1] != nt
    if not bad and nt:
        bad = pix.min() < 0 or pix.max() >= b * h * w or (np.diff(pix) <= 0).any() \
            or (pix // (h * w) != np.repeat(np.arange(b), np.diff(img_seg))).any()
    if not bad and ent.size:
        bad = ent.min() < 0 or ent.max() >= rows * 9
    if bad:
        raise _lib.FgnHipError('guidance_backward: the index does not fit the operands')
    packed = np.concatenate([pix, seg, ent, img_seg])
    dev_idx = torch.from_numpy(packed).to(taps.device, non_blocking=True) if upload is None else upload(packed)
    _chk(dev_idx, 'index', torch.int32)
    o1, o2, o3 = nt, nt + seg.size, nt + seg.size + ent.size
    if out is None:
        out = torch.empty_like(qry_fmap)
        accumulate = False
    else:
        _chk(out, 'out')
        if out.shape != qry_fmap.shape:
            raise _lib.FgnHipError('guidance_backward: bad out shape')
    slab = torch.empty((max(nt, 1), n, c), device=taps.device, dtype=torch.float32)
    d_vec = torch.empty_like(vec)
    rc = _lib.load().fgn_guidance_backward_f32(_ptr(taps), _ptr(dev_idx[:o1]), _ptr(dev_idx[o1:o2]), _ptr(dev_idx[o2:o3]),
                                               _ptr(dev_idx[o3:]), _ptr(qry_fmap), _ptr(vec), _ptr(out), _ptr(slab),
                                               _ptr(d_vec), nt, b, n, h * w, c, int(accumulate), _stream())
    _lib.check(rc, 'fgn_guidance_backward_f32')
    return out, d_vec


def adagrad_multi(params, grads, states, lrs, weight_decay: float, eps: float = 1e-10, table: Optional[dict] = None) -> None:
    """``adagrad_step`` for a list of tensors in one launch (each with its own learning rate).  ``table``: a dict the
    caller keeps between steps - the checked parameter / state pointer arrays are built once per (tensors, lrs) and only
    the gradient pointers are refreshed (the parameters of a ``Trainer`` never move)."""
    import ctypes as C
    k = len(params)
    if not (len(grads) == len(states) == len(lrs) == k):
        raise _lib.FgnHipError('adagrad_multi: list lengths differ')
    if not k:
        return
    key = (tuple(p.data_ptr() for p in params), tuple(s.data_ptr() for s in states), tuple(float(v) for v in lrs))
    if table is None or table.get('key') != key:
        for p, s in zip(params, states):
            _chk(p, 'param'); _chk(s, 'state')
            if not (p.is_contiguous() and s.is_contiguous()) or s.numel() != p.numel():
                raise _lib.FgnHipError('adagrad_multi: parameters and states must be contiguous and of equal size')
        built = dict(key=key, pa=(C.c_void_p * k)(*key[0]), sa=(C.c_void_p * k)(*key[1]),
                     na=(C.c_longlong * k)(*[p.numel() for p in params]), la=(C.c_float * k)(*key[2]),
                     ga=(C.c_void_p * k)(), numel=[p.numel() for p in params])
        if table is None:
            table = built
        else:
            table.clear(); table.update(built)
    ga = table['ga']
    for i, g in enumerate(grads):
        if not g.is_cuda or g.dtype != torch.float32 or not g.is_contiguous() or g.numel() != table['numel'][i]:
            raise _lib.FgnHipError('adagrad_multi: gradients must be contiguous fp32 device tensors of the parameters\' sizes')
        ga[i] = g.data_ptr()
    rc = _lib.load().fgn_adagrad_multi_f32(table['pa'], ga, table['sa'], table['na'], table['la'], k, float(weight_decay),
                                           float(eps), _stream())
    _lib.check(rc, 'fgn_adagrad_multi_f32')


def adagrad_step(param: torch.Tensor, grad: torch.Tensor, state: torch.Tensor, lr: float, weight_decay: float,
                 eps: float = 1e-10) -> None:
    for t, nm in ((param, 'param'), (grad, 'grad'), (state, 'state')):
        _chk(t, nm)
    if grad.numel() != param.numel() or state.numel() != param.numel():
        raise _lib.FgnHipError('adagrad_step: operand sizes differ')
    rc = _lib.load().fgn_adagrad_step_f32(_ptr(param), _ptr(grad), _ptr(state), param.numel(), float(lr),
                                          float(weight_decay), float(eps), _stream())
    _lib.check(rc, 'fgn_adagrad_step_f32')


# --------------------------------------------------------------------------------------
# optimiser rules, gradient norm and accumulation over tensor lists (csrc/optim.hip)
OPTIM_RULES = {'Adagrad': 0, 'Adam': 1, 'SGD': 2}
OPTIM_CHUNK = 4096


def _list_ptrs(tensors, name: str, numel=None):
    """-> ctypes pointer array of a list of contiguous fp32 device tensors (checked; ``numel``: the sizes they must have)."""
    import ctypes as C
    arr = (C.c_void_p * max(len(tensors), 1))()
    for i, t in enumerate(tensors):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() \
                or (numel is not None and t.numel() != numel[i]):
            raise _lib.FgnHipError(f'{name}: entry {i} must be a contiguous fp32 device tensor of its parameter\'s size')
        arr[i] = t.data_ptr()
    return arr


def optim_multi(rule: str, params, grads, states, lrs, weight_decay: float = 0.0, eps: Optional[float] = None,
                betas=(0.9, 0.999), step: int = 1, momentum: float = 0.0, nesterov: bool = False, dampening: float = 0.0,
                coef: Optional[torch.Tensor] = None, grad_scale: float = 1.0, table: Optional[dict] = None) -> None:
    """One optimiser step of ``rule`` ('Adagrad' | 'Adam' | 'SGD': torch.optim's single-tensor forms) on a list of tensors
    in one launch per 64 non-empty tensors, each tensor with its own learning rate.

    ``states``: per tensor the Adagrad ``sum``, the Adam pair ``(exp_avg, exp_avg_sq)`` or the SGD ``momentum_buffer``
    (``None`` for the whole list when ``momentum`` is 0).  ``step``: the number of optimiser steps taken including this
    one (Adam's bias corrections, formed here in double from the fp32 betas).  The gradient enters as
    ``g * coef * grad_scale``: ``coef`` is the device record of ``grad_norm_multi`` (its second element is read by the
    kernel, no host synchronisation), ``grad_scale`` a host scalar; with ``coef=None`` and ``grad_scale=1`` the gradient
    is used bit for bit.  ``table``: a dict the caller keeps between steps - the checked parameter / state pointer arrays
    are built once per (tensors, lrs) and only the gradient pointers are refreshed."""
    import ctypes as C
    if rule not in OPTIM_RULES:
        raise _lib.FgnHipError(f'optim_multi: unknown rule {rule!r} (one of {sorted(OPTIM_RULES)})')
    if float(dampening) != 0.0:
        raise _lib.FgnHipError('optim_multi: SGD dampening other than 0 is not supported')
    k = len(params)
    no_state = rule == 'SGD' and float(momentum) == 0.0
    if states is None:
        if not no_state:
            raise _lib.FgnHipError(f'optim_multi: {rule} needs its state tensors')
        states = [None] * k
    if not (len(grads) == len(states) == len(lrs) == k):
        raise _lib.FgnHipError('optim_multi: list lengths differ')
    if not k:
        return
    if rule == 'Adam':
        s1 = [s[0] for s in states]
        s2 = [s[1] for s in states]
    else:
        s1, s2 = (None if no_state else list(states)), None
    key = (rule, tuple(p.data_ptr() for p in params), tuple(s.data_ptr() for s in s1) if s1 else None,
           tuple(s.data_ptr() for s in s2) if s2 else None, tuple(float(v) for v in lrs))
    if table is None or table.get('key') != key:
        numel = [p.numel() for p in params] if all(torch.is_tensor(p) for p in params) else None
        built = dict(key=key, pa=_list_ptrs(params, 'optim_multi: params'),
                     s1=_list_ptrs(s1, 'optim_multi: states', numel) if s1 else None,
                     s2=_list_ptrs(s2, 'optim_multi: states', numel) if s2 else None,
                     na=(C.c_longlong * k)(*numel), la=(C.c_float * k)(*key[4]), ga=(C.c_void_p * k)(), numel=numel)
        if table is None:
            table = built
        else:
            table.clear(); table.update(built)
    ga = table['ga']
    for i, g in enumerate(grads):
        if not torch.is_tensor(g) or not g.is_cuda or g.dtype != torch.float32 or not g.is_contiguous() \
                or g.numel() != table['numel'][i]:
            raise _lib.FgnHipError('optim_multi: gradients must be contiguous fp32 device tensors of the parameters\' sizes')
        ga[i] = g.data_ptr()
    if coef is not None:
        _chk(coef, 'coef')
        if coef.numel() != 2:
            raise _lib.FgnHipError('optim_multi: coef is the {norm, coef} record of grad_norm_multi')
    if eps is None:
        eps = 1e-8 if rule == 'Adam' else 1e-10
    h0 = h1 = 0.0
    bc1 = bc2 = 1.0
    if rule == 'Adam':
        if int(step) < 1:
            raise _lib.FgnHipError('optim_multi: Adam step counts from 1')
        h0, h1 = (float(C.c_float(b).value) for b in betas)
        bc1, bc2 = 1.0 - h0 ** int(step), 1.0 - h1 ** int(step)
    elif rule == 'SGD':
        h0 = float(momentum)
    rc = _lib.load().fgn_optim_multi_f32(OPTIM_RULES[rule], table['pa'], ga, table['s1'], table['s2'], table['na'],
                                         table['la'], k, float(weight_decay), float(eps), h0, h1, bc1, bc2,
                                         int(bool(nesterov)), None if coef is None else coef.data_ptr() + 4,
                                         float(grad_scale), _stream())
    _lib.check(rc, 'fgn_optim_multi_f32')


def grad_norm_multi(grads, max_norm: float, norm_type: float = 2, out: Optional[torch.Tensor] = None,
                    grad_scale: float = 1.0) -> torch.Tensor:
    """The global L2 norm of a list of gradients and the coefficient of ``torch.nn.utils.clip_grad_norm_(max_norm,
    norm_type=2)`` -> device record ``out`` = [norm, coef], norm that of ``grad_scale * g`` (the host scalar
    ``optim_multi`` multiplies the gradients by), coef = min(1, max_norm / (norm + 1e-6)); nothing is scaled
    here - ``optim_multi(coef=out)`` applies the coefficient.  Squares are summed in fp64 in a fixed order without
    atomics (the same input gives the same bits); no host synchronisation.  Non-finite gradients behave as in torch with
    ``error_if_nonfinite=False``: the norm and the coefficient become NaN, and so do the gradients they multiply."""
    import ctypes as C
    if float(norm_type) != 2.0:
        raise _lib.FgnHipError(f'grad_norm_multi: norm_type {norm_type} is not supported (2 only)')
    if not float(max_norm) >= 0.0:
        raise _lib.FgnHipError('grad_norm_multi: max_norm must be >= 0')
    k = len(grads)
    ga = _list_ptrs(grads, 'grad_norm_multi: grads')
    dev = grads[0].device if k else torch.device('cuda', torch.cuda.current_device())
    if out is None:
        out = torch.empty(2, device=dev, dtype=torch.float32)
    else:
        _chk(out, 'out')
        if out.numel() != 2:
            raise _lib.FgnHipError('grad_norm_multi: out holds {norm, coef}')
    na = (C.c_longlong * max(k, 1))(*[g.numel() for g in grads])
    chunks = sum((g.numel() + OPTIM_CHUNK - 1) // OPTIM_CHUNK for g in grads)
    part = torch.empty(max(chunks, 1), device=dev, dtype=torch.float64)
    rc = _lib.load().fgn_grad_sqnorm_multi_f32(ga, na, k, float(max_norm), float(grad_scale), part.data_ptr(), part.numel(), out.data_ptr(),
                                               _stream())
    _lib.check(rc, 'fgn_grad_sqnorm_multi_f32')
    return out


def grad_accumulate_multi(accs, grads, a: float, first: bool) -> None:
    """``acc = (0 if first else acc) + a * g`` over a list of tensors in one launch per 64 non-empty tensors; ``first``
    overwrites whatever the accumulators held (no zero fill needed)."""
    import ctypes as C
    k = len(accs)
    if len(grads) != k:
        raise _lib.FgnHipError('grad_accumulate_multi: list lengths differ')
    if not k:
        return
    aa = _list_ptrs(accs, 'grad_accumulate_multi: accs')
    numel = [t.numel() for t in accs]
    ga = _list_ptrs(grads, 'grad_accumulate_multi: grads', numel)
    rc = _lib.load().fgn_grad_accumulate_multi_f32(aa, ga, (C.c_longlong * k)(*numel), k, float(a), int(bool(first)),
                                                   _stream())
    _lib.check(rc, 'fgn_grad_accumulate_multi_f32')
