"""The binding's contract, wrapper by wrapper, WITHOUT a GPU and without a kernel launch (DESIGN.md "The binding's contract").

hip.py is the only place where a torch tensor becomes a raw pointer plus a few integers, so its checks are the whole guard of the kernels.  Here the
library is replaced by a stub that forwards the host-only entry points to the real one and records, without running it, every compute entry point
reached.  One row per wrapper: a valid call at the smallest shape that exercises its arguments, and mutations that each break ONE claim.  A valid call
must reach exactly its entry points and hand back the documented shapes and dtypes; a mutated call must raise MrdisError before any entry point.
The refusal cases must never meet real kernels (a wrong check would hand a kernel a bad buffer): nothing here is marked gpu, and there is no GPU twin.

Hot wrappers (what a training step calls) check shapes and element counts inline (the dtype where the entry point takes no storage code) and leave out
per-operand device compares, and for parameter and statistics vectors the density compare as well (each compare is host time on every call); the cold ones
(per subject / volume / file) check the device too: their rows carry a 'meta' mutation, a tensor of the right shape on another device.
"""
import inspect
import os
import re
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import mrdis                                                    # noqa: E402

hip = mrdis.hip
F32, F64, BF16, I32, I64, U8 = torch.float32, torch.float64, torch.bfloat16, torch.int32, torch.int64, torch.uint8
HOST_ONLY_NAMES = {'mrdis_wino_u_format', 'mrdis_wino_u_image_floats', 'mrdis_wino_u_image_floats_fmt', 'mrdis_strerror', 'mrdis_version', 'mrdis_set_option',
                   'mrdis_get_option', 'mrdis_launch_count', 'mrdis_launch_count_reset', 'mrdis_dynamic_lds_table'}


def host_only(name):
    if name == 'mrdis_copy_bytes':          # a kernel, whatever its name ends in
        return False
    return name.endswith(('_workspace', '_bytes', '_blocks', '_applies')) or name in HOST_ONLY_NAMES


COMPUTE = {n for n in hip._SIGS if not host_only(n)}


class StubLibrary:
    """host-only entry points go to the real library (it loads without a GPU); every other symbol is recorded and answers MRDIS_OK"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if name not in hip._SIGS:
            raise AttributeError(name)
        if host_only(name):
            return getattr(self.real, name)

        def record(*args):
            self.calls.append(name[len('mrdis_'):])
            return 0
        return record


def install_stub(setattr_):
    stub = StubLibrary(hip.load())
    setattr_(hip, '_lib', stub)
    setattr_(hip, 'load', lambda path=None: stub)
    setattr_(hip, '_stream', lambda: 0)
    return stub


# ---------------------------------------------------------------- operands
def z(*shape, dtype=F32):
    return torch.zeros(shape, dtype=dtype)


def cl(*shape, dtype=F32):
    """a dense channels-last (B, C, H, W) / channels-last-3d (B, C, D, H, W) tensor"""
    return torch.zeros(shape, dtype=dtype).contiguous(memory_format=torch.channels_last if len(shape) == 4 else torch.channels_last_3d)


def vol(*shape):
    return torch.zeros(shape or (1, 4, 5, 6), dtype=U8)


# mutations: each takes the keyword arguments of the valid call and breaks one claim in place
def short(k):
    """one row short"""
    return lambda kw: kw.__setitem__(k, kw[k][:-1])


def to(k, dtype):
    return lambda kw: kw.__setitem__(k, kw[k].to(dtype))


def meta(k):
    """the right shape on another device"""
    return lambda kw: kw.__setitem__(k, kw[k].to('meta'))


def strided(k):
    """the right shape, but every second element of a wider buffer: not dense"""
    return lambda kw: kw.__setitem__(k, torch.stack([kw[k], kw[k]], dim=-1)[..., 0])


def put(k, make):
    return lambda kw: kw.__setitem__(k, make())


def item(k, i, f):
    """mutate element i of a list argument"""
    def go(kw):
        sub = {0: kw[k][i]}
        f(0)(sub)
        kw[k] = list(kw[k]); kw[k][i] = sub[0]
    return go


X = (2, 8, 5, 6)                      # the 2-D family: N = 2, C = 8, 5 x 6 maps
X4 = (2, 4, 5, 6)                     # ... where the four-channel forms differ
V = (2, 8, 3, 4, 5)                   # the 3-D family
CONV = dict(kh=3, kw=3, stride=1, pad=1)
C3 = dict(k=3, stride=1, pad=1)
W5 = (3, 8, 4, 3, 3)                  # expert filters (E, Co, Ci, kh, kw)
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=1, max_norm=1.0)


def JOB(struct):
    """a table of one job struct"""
    import ctypes
    return z(ctypes.sizeof(getattr(hip, struct)), dtype=U8)


# name -> (valid keyword arguments, entry points reached, [(shape, dtype)] of the flattened tensor results, {what breaks: mutation})
ROWS = {
    'stream_fill': (lambda: dict(t=z(8)), ['stream_fill'], [((8,), F32)], {'not dense': strided('t'), 'dtype': to('t', I32), 'not a multiple of 4': short('t')}),
    'copy_bytes': (lambda: dict(src=z(4), dst=z(4), nbytes=16), ['copy_bytes'], [], {'past the end': put('nbytes', lambda: 20), 'odd size': put('nbytes', lambda: 6)}),
    's6_filter_image': (lambda: dict(w=z(9, 16, 16)), ['s6_filter_image'], [((27648 // 4,), F32)], {'not a filter': put('w', lambda: z(9, 16))}),
    'wino_u_jobs': (lambda: dict(table=JOB('WinoUJob'), njobs=1, total_blocks=1), ['wino_u_jobs'], [], {'table too short': put('njobs', lambda: 2), 'dtype': to('table', I32)}),
    'mix_jobs_fwd': (lambda: dict(table=JOB('MixJob'), njobs=1, total_blocks=1, types=z(4, 3)), ['mix_jobs_fwd'], [],
                     {'table too short': put('njobs', lambda: 2), 'dtype': to('types', F64), 'not dense': strided('types')}),
    'mix_jobs_bwd': (lambda: dict(table=JOB('MixJob'), njobs=1, total_blocks=1, dw_table=z(1, 8, dtype=I64), types=z(4, 3)), ['mix_jobs_bwd'], [],
                     {'dw_table short': put('dw_table', lambda: z(7, dtype=I64)), 'dw_table not dense': strided('dw_table'), 'table too short': put('njobs', lambda: 2), 'dtype': to('types', F64), 'not dense': strided('types')}),
    'cast_view': (lambda: dict(x=cl(*X), dtype=BF16), ['cast_view'], [(X, BF16)], {'dtype': to('x', F64), 'not 4-d': put('x', lambda: z(8, 5, 6))}),
    'cast_bf16': (lambda: dict(t=z(4, 4)), ['cast_bf16'], [((4, 4), BF16)], {'dtype': to('t', F64)}),
    'mix_experts_fwd': (lambda: dict(W=z(*W5), r=z(3)), ['mix_experts_fwd'], [((9, 4, 8), F32), ((9, 8, 4), F32)], {'r short': short('r'), 'dtype': to('W', F64)}),
    'mix_experts_bwd': (lambda: dict(dw_tck=z(9, 4, 8), W=z(*W5), r=z(3)), ['mix_experts_bwd'], [(W5, F32), ((3,), F32)],
                        {'dw short': short('dw_tck'), 'r short': short('r'), 'dtype': to('dw_tck', F64)}),
    'mix_experts_routed_fwd': (lambda: dict(W=z(*W5), fcw=z(3, 5), fcb=z(3), t_row=z(1, 5)), ['mix_experts_routed_fwd'], [((9, 4, 8), F32), ((9, 8, 4), F32), ((3,), F32)],
                               {'fcb short': short('fcb'), 't_row short': put('t_row', lambda: z(1, 4)), 'dtype': to('fcw', F64)}),
    'mix_experts_routed_bwd': (lambda: dict(dw_tck=z(9, 4, 8), W=z(*W5), r=z(3), t_row=z(1, 5), emb=5), ['mix_experts_routed_bwd'], [(W5, F32), ((3, 5), F32), ((3,), F32)],
                               {'r short': short('r'), 'dw short': short('dw_tck'), 't_row short': put('t_row', lambda: z(1, 4))}),
    'mix_experts_routed_multi_fwd': (lambda: dict(W=z(*W5), fcw=z(3, 5), fcb=z(3), types=z(4, 5)), ['mix_experts_routed_multi_fwd'],
                                     [((9, 4, 8), F32)] * 4 + [((9, 8, 4), F32)] * 4 + [((4, 3), F32)],
                                     {'fcb short': short('fcb'), 'types narrower than fcw': put('types', lambda: z(4, 4)),
                                      'into: a list one filter short': put('into', lambda: ([z(9, 4, 16)] * 3, [z(9, 16, 4)] * 4, None, None, 0, 16)),
                                      'into: columns past the filter': put('into', lambda: ([z(9, 4, 16)] * 4, [z(9, 16, 4)] * 4, None, None, 9, 16))}),
    'mix_experts_routed_multi_bwd': (lambda: dict(dw_list=[z(9, 4, 8) for _ in range(4)], W=z(*W5), r=z(4, 3), types=z(4, 5)), ['mix_experts_routed_multi_bwd'],
                                     [(W5, F32), ((3, 5), F32), ((3,), F32)],
                                     {'r short': short('r'), 'a gradient short': item('dw_list', 0, short), 'a gradient missing': put('dw_list', lambda: [z(9, 4, 8)] * 3),
                                      'sink short': put('sinks', lambda: (z(*W5), z(3, 4), z(3)))}),
    'conv2d_fwd': (lambda: dict(x=cl(*X), w_tck=z(9, 8, 4), bias=z(4), **CONV), ['conv2d_fwd'], [(X4, F32)],
                   {'filter channels': put('w_tck', lambda: z(9, 7, 4)), 'filter taps': put('w_tck', lambda: z(8, 8, 4)), 'bias short': short('bias'),
                    'out shape': put('out', lambda: cl(2, 4, 5, 5)), 'out not NHWC': put('out', lambda: z(*X4)),
                    'x dtype': to('x', F64), 'w_bf16 shape': put('w_bf16', lambda: z(9, 4, 7, dtype=BF16))}),
    'conv2d_bwd_data': (lambda: dict(dy=cl(*X4), w_tkc=z(9, 4, 8), in_hw=(5, 6), **CONV), ['conv2d_bwd_data'], [(X, F32)],
                        {'filter channels': put('w_tkc', lambda: z(9, 3, 8)), 'filter taps': put('w_tkc', lambda: z(8, 4, 8)), 'input size': put('in_hw', lambda: (6, 6)),
                         'out shape': put('out', lambda: cl(2, 8, 5, 5)), 'w_bf16 shape': put('w_bf16', lambda: z(9, 8, 3, dtype=BF16))}),
    'conv2d_bwd_weight': (lambda: dict(x=cl(*X), dy=cl(*X4), **CONV), ['conv2d_bwd_weight'], [((9, 8, 4), F32), ((4,), F32)],
                          {'dy short': short('dy'), 'dy size': put('dy', lambda: cl(2, 4, 4, 6)), 'bias_sink short': put('bias_sink', lambda: z(3)), 'dy dtype': to('dy', F64)}),
    'lrelu_bwd': (lambda: dict(dy=cl(*X), y=cl(*X)), ['lrelu_bwd'], [(X, F32)], {'dy short': short('dy'), 'dy dtype': to('dy', F64), 'mixed storage': to('dy', BF16)}),
    'bn_train_fwd': (lambda: dict(x=cl(*X), gamma=z(8), beta=z(8), running_mean=z(8), running_var=z(8), eps=1e-5, momentum=0.1), ['bn_train_fwd'],
                     [(X, F32), ((8,), F32), ((8,), F32)],
                     {'gamma short': short('gamma'), 'running_var short': short('running_var'), 'running_var dtype': to('running_var', BF16), 'out shape': put('out', lambda: cl(2, 8, 5, 5)),
                      'groups': put('groups', lambda: 3)}),
    'bn_eval_fwd': (lambda: dict(x=cl(*X), gamma=z(8), beta=z(8), running_mean=z(8), running_var=z(8), eps=1e-5), ['bn_eval_fwd'], [(X, F32)],
                    {'gamma short': short('gamma'), 'beta short': short('beta'), 'running_mean short': short('running_mean'), 'running_var short': short('running_var'), 'gamma dtype': to('gamma', BF16)}),
    'bn_train_bwd': (lambda: dict(dy=cl(*X), x=cl(*X), gamma=z(8), mean=z(8), rstd=z(8)), ['bn_train_bwd'], [(X, F32), ((8,), F32), ((8,), F32)],
                     {'dy short': short('dy'), 'gamma short': short('gamma'), 'mean short': short('mean'), 'rstd short': short('rstd'),
                      'sink short': put('sink', lambda: (z(7), z(8))), 'rstd dtype': to('rstd', BF16)}),
    'instnorm_spade_fwd': (lambda: dict(z=cl(*X), gamma=cl(*X), beta=cl(*X)), ['instnorm_spade_fwd'], [(X, F32), ((16,), F32), ((16,), F32)],
                           {'gamma short': short('gamma'), 'beta short': short('beta'), 'stats short': put('stats', lambda: (z(15), z(16))), 'beta dtype': to('beta', BF16)}),
    'gb_spade_fwd': (lambda: dict(si_out=cl(*X), w_tck=z(9, 8, 16), bias=z(16), z=cl(*X)), ['instnorm_stats', 'conv2d_fwd_spade'], [(X, F32), (X, F32), ((16,), F32), ((16,), F32)],
                     {'bias short': short('bias'), 'w_bf16 size': put('w_bf16', lambda: z(9, 16, 7, dtype=BF16)), 'out shape': put('out', lambda: (cl(2, 8, 5, 5), cl(*X), z(16), z(16))),
                      'out statistics short': put('out', lambda: (cl(*X), cl(*X), z(15), z(16)))}),
    'instnorm_spade_bwd': (lambda: dict(dout=cl(*X), z=cl(*X), gamma=cl(*X), mean=z(16), rstd=z(16)), ['instnorm_spade_bwd'], [(X, F32), (X, F32)],
                           {'dout short': short('dout'), 'z short': short('z'), 'mean short': short('mean'), 'rstd short': short('rstd'), 'rstd dtype': to('rstd', BF16),
                            'up2 without fused_gb': put('up2', lambda: True)}),
    'bilinear_fwd': (lambda: dict(x=cl(*X), out_hw=(10, 12), align_corners=False), ['bilinear_fwd'], [((2, 8, 10, 12), F32)], {'dtype': to('x', F64)}),
    'bilinear_up2_stats': (lambda: dict(x=cl(*X), eps=1e-5), ['bilinear_up2_stats_fwd'], [((2, 8, 10, 12), F32), ((16,), F32), ((16,), F32)],
                           {'dtype': to('x', F64), 'out_blocks shape': put('out_blocks', lambda: z(1, 2, 8, 10, 11)), 'out_blocks not NHWC': put('out_blocks', lambda: z(1, 2, 8, 10, 12))}),
    'bilinear_bwd': (lambda: dict(dy=cl(2, 8, 10, 12), in_hw=(5, 6), align_corners=False), ['bilinear_bwd'], [(X, F32)],
                     {'dtype': to('dy', F64), 'out shape': put('out', lambda: cl(2, 8, 5, 5)), 'out dtype': put('out', lambda: cl(*X, dtype=BF16))}),
    'softmax_mask_drop_fwd': (lambda: dict(s=cl(*X4), mask_img=z(2, 5, 6)), ['softmax_mask_drop_fwd'], [(X4, F32)],
                              {'mask short': short('mask_img'), 'mask dtype': to('mask_img', F64), 'bf16 scores': to('s', BF16)}),
    'softmax_mask_drop_bwd': (lambda: dict(dout=cl(*X4), out=cl(*X4)), ['softmax_mask_drop_bwd'], [(X4, F32)], {'dout short': short('dout'), 'bf16': to('out', BF16)}),
    'recon_err_fwd': (lambda: dict(gt=cl(*X4), x=cl(*X4), p=1), ['recon_err_fwd'], [((2,), F32)], {'gt short': short('gt'), 'bf16': to('gt', BF16)}),
    'recon_err_bwd': (lambda: dict(gt=cl(*X4), x=cl(*X4), w=z(2), p=1), ['recon_err_bwd'], [(X4, F32)], {'gt short': short('gt'), 'w short': short('w'), 'w dtype': to('w', F64)}),
    'recon_metrics': (lambda: dict(target=cl(2, 1, 8, 8), pred=cl(2, 1, 8, 8)), ['recon_metrics'], [((2, 3), F32)], {'target short': short('target'), 'bf16': to('pred', BF16)}),
    'slice_gather': (lambda: dict(vol_ptrs=z(2, 4, dtype=I64), slice_idx=z(2, dtype=I32), drop=z(2, dtype=I32), H=5, W=6, D=7, block=1), ['slice_gather'],
                     [((2, 12, 5, 6), F32), ((2, 4), F32), ((2, 5, 6), F32)],
                     {'slice_idx short': short('slice_idx'), 'drop dtype': to('drop', I64), 'vol_ptrs dtype': to('vol_ptrs', I32), 'vol_ptrs not dense': strided('vol_ptrs'),
                      'drop on another device': meta('drop')}),
    'volume_gather': (lambda: dict(table=z(2, 11, dtype=I64), M=4, H=4, W=5, D=6, z0=0, Dz=6), ['volume_gather'], [((2, 4, 4, 5, 6), F32), ((2, 4), F32)],
                      {'dtype': to('table', I32), 'rows short': put('table', lambda: z(2, 10, dtype=I64)), 'not dense': strided('table')}),
    'nvnet_loss_fwd': (lambda: dict(uout=z(2, 3, 4, 5, 6), target=z(2, 3, 4, 5, 6)), ['nvnet_loss_fwd'], [((4,), F64), ((3,), F32)],
                       {'target short': short('target'), 'dtype': to('target', F64), 'target on another device': meta('target'), 'vout without x': put('vout', lambda: z(2, 4))}),
    'nvnet_loss_bwd': (lambda: dict(g=torch.ones(()), sums=z(4, dtype=F64), uout=z(2, 3, 4, 5, 6), target=z(2, 3, 4, 5, 6)), ['nvnet_loss_bwd'], [((2, 3, 4, 5, 6), F32)],
                       {'sums dtype': to('sums', F32), 'sums short': short('sums'), 'target short': short('target'), 'g dtype': to('g', F64),
                        'sums on another device': meta('sums')}),
    'seg_counts': (lambda: dict(pred=cl(2, 3, 4, 5, 6), target=cl(2, 3, 4, 5, 6)), ['seg_counts'], [((2, 3, 3), I32)],
                   {'target short': short('target'), 'dtype': to('target', F64), 'target on another device': meta('target')}),
    'seg_accum': (lambda: dict(logits=cl(2, 3, 4, 5, 6), acc=z(2, 4, 5, 7, 3), z0=0), ['seg_accum'], [((2, 4, 5, 7, 3), F32)],
                  {'logits not channels-last': put('logits', lambda: z(2, 3, 4, 5, 6)), 'acc shape': put('acc', lambda: z(2, 4, 5, 7, 2)), 'acc dtype': to('acc', F64),
                   'acc not dense': strided('acc'), 'acc on another device': meta('acc')}),
    'seg_label_volume': (lambda: dict(acc=z(2, 4, 5, 7, 3), cover=z(7, dtype=I32)), ['seg_label_volume'], [((2, 4, 5, 7), U8), ((2, 3, 3), I32)],
                         {'cover short': short('cover'), 'cover dtype': to('cover', I64), 'cover on another device': meta('cover'), 'acc not dense': strided('acc'),
                          'target_ptrs long': put('target_ptrs', lambda: z(3, dtype=I64)), 'target_ptrs on another device': put('target_ptrs', lambda: z(2, dtype=I64).to('meta'))}),
    'region_surfaces': (lambda: dict(labels=vol(), target_ptrs=None, region_masks=[2, 6]), ['region_surfaces'], [((1, 4, 5, 6), U8), ((1, 2, 5), I32)],
                        {'dtype': to('labels', I32), 'not dense': strided('labels'), 'target_ptrs long': put('target_ptrs', lambda: z(2, dtype=I64)),
                         'target_ptrs on another device': put('target_ptrs', lambda: z(1, dtype=I64).to('meta')), 'five regions': put('region_masks', lambda: [2] * 5)}),
    'edt_sq': (lambda: dict(src=vol()), ['edt_sq'], [((1, 1, 4, 5, 6), I32)], {'dtype': to('src', I32), 'not 4-d': put('src', lambda: vol(4, 5, 6)), 'not dense': strided('src')}),
    'surface_hist': (lambda: dict(flags=vol(), R=2), ['surface_hist'], [((1, 2, 2, hip.edt_bins(4, 5, 6)), I32)], {'dtype': to('flags', I32), 'five regions': put('R', lambda: 5)}),
    'cc_label': (lambda: dict(labels=vol(), fg_mask=0b10110), ['cc_label'], [((1, 4, 5, 6), I32)] * 2,
                 {'dtype': to('labels', I32), 'not dense': strided('labels'), 'background in the mask': put('fg_mask', lambda: 1)}),
    'cc_clean': (lambda: dict(labels=vol(), comp=z(1, 4, 5, 6, dtype=I32), size=z(1, 4, 5, 6, dtype=I32)), ['cc_clean'], [((1, 4, 5, 6), U8), ((1, 6), I32)],
                 {'comp dtype': to('comp', I64), 'size shape': put('size', lambda: z(1, 4, 5, 5, dtype=I32)), 'comp on another device': meta('comp'), 'size not dense': strided('size')}),
    'synth_accum': (lambda: dict(recons=[cl(2, 3, 5, 6)], centres=[3, 4], acc=z(7, 5, 6), cnt=z(7, dtype=I32), c_lo=1, c_hi=1), ['synth_accum'], [((7, 5, 6), F32)],
                    {'source not channels-last': put('recons', lambda: [z(2, 3, 5, 6)]), 'cnt short': short('cnt'), 'cnt on another device': meta('cnt'),
                     'acc dtype': to('acc', F64), 'a gap in the centres': put('centres', lambda: [3, 5]), 'source on another device': item('recons', 0, meta)}),
    'synth_finish': (lambda: dict(acc=z(7, 5, 6), cnt=z(7, dtype=I32)), ['synth_finish'], [((7, 5, 6), F32), ((5, 6, 7), F32)],
                     {'cnt short': short('cnt'), 'cnt on another device': meta('cnt'), 'acc not dense': strided('acc'), 'cnt dtype': to('cnt', I64)}),
    # prep_stats, prep_write and export_volume demand a device tensor: only their refusals run here (tests/test_gpu_prep.py and test_gpu_export.py hold the valid calls)
    'prep_stats': (lambda: dict(raw=z(4, 6, 8, dtype=torch.int16), crop=((0, 0), (0, 0))), None, None, {'raw on the host': lambda kw: None}),
    'prep_write': (lambda: dict(raw=z(4, 6, 8, dtype=torch.int16), stats=z(5, dtype=F64), kind='zscore', crop=((0, 0), (0, 0)), layout='dhw'), None, None,
                   {'raw on the host': lambda kw: None}),
    'export_volume': (lambda: dict(src=vol(4, 6, 8), crop=((0, 0), (0, 0)), layout='hwd'), None, None, {'src on the host': lambda kw: None, 'crop': put('crop', lambda: (1, 2))}),
    'seg2d_label_planes': (lambda: dict(views=[[cl(2, 3, 5, 6)]], flips=[0], planes=vol(1, 7, 5, 6), s0=1), ['seg2d_label_planes'], [((1, 7, 5, 6), U8)],
                           {'view not channels-last': put('views', lambda: [[z(2, 3, 5, 6)]]), 'planes dtype': to('planes', I32), 'a set too many': put('planes', lambda: vol(2, 7, 5, 6)),
                            'past the volume': put('s0', lambda: 6), 'view on another device': put('views', lambda: [[cl(2, 3, 5, 6).to('meta')]])}),
    'seg2d_finish': (lambda: dict(planes=vol(1, 7, 5, 6)), ['seg2d_finish'], [((1, 5, 6, 7), U8)], {'dtype': to('planes', I32), 'not dense': strided('planes')}),
    'fuse_present_fwd': (lambda: dict(srcs=[cl(*X4), cl(*X4)], mask=torch.ones(2, 2), method='mean'), ['fuse_present_fwd'], [(X4, F32)],
                         {'mask narrow': put('mask', lambda: torch.ones(2, 1)), 'mask on another device': meta('mask'), 'a map short': item('srcs', 1, short),
                          'a map dtype': item('srcs', 1, lambda k: to(k, F64)), 'out shape': put('out', lambda: cl(2, 4, 5, 5)), 'a map on another device': item('srcs', 1, meta)}),
    'fuse_present_bwd': (lambda: dict(dout=cl(*X4), srcs=[cl(*X4), cl(*X4)], mask=torch.ones(2, 2), method='mean'), ['fuse_present_bwd'], [(X4, F32)] * 2,
                         {'dout short': short('dout'), 'dout on another device': meta('dout'), 'a gradient view missing': put('outs', lambda: [cl(*X4)]),
                          'a gradient view shape': put('outs', lambda: [cl(*X4), cl(2, 4, 5, 5)])}),
    'maxpool_fwd': (lambda: dict(x=cl(2, 8, 4, 6), k=2), ['maxpool_fwd'], [((2, 8, 2, 3), F32), ((2, 2, 3, 8), I32)], {'bf16': to('x', BF16), 'window': put('k', lambda: 0)}),
    'maxpool_bwd': (lambda: dict(dy=cl(2, 8, 2, 3), arg=z(2, 2, 3, 8, dtype=I32), in_shape=(2, 8, 4, 6), k=2), ['maxpool_bwd'], [((2, 8, 4, 6), F32)],
                    {'argmax dtype': to('arg', I64), 'argmax short': short('arg'), 'dy short': short('dy'), 'argmax not dense': strided('arg')}),
    'sumsq_finite': (lambda: dict(g=z(16), out=z(2)), ['sumsq_finite'], [], {'dtype': to('g', F64), 'out short': short('out'), 'not dense': strided('g')}),
    'adam_amsgrad_step': (lambda: dict(p=z(16), g=z(16), m=z(16), v=z(16), vmax=z(16), norm_finite=z(2), **ADAM), ['adam_amsgrad_step'], [],
                          {'g short': short('g'), 'm dtype': to('m', F64), 'vmax not dense': strided('vmax'), 'norm_finite short': short('norm_finite'),
                           'a gate past the arena': put('gates', lambda: ([(8, 17)], [0], torch.ones(1))), 'a flag index past the flags': put('gates', lambda: ([(0, 8)], [1], torch.ones(1))),
                           'gate_steps short': lambda kw: kw.update(step_state=z(2), gates=([(0, 8)], [1], torch.ones(2)), gate_steps=z(3)),
                           'gate_steps without step_state': lambda kw: kw.update(gates=([(0, 8)], [0], torch.ones(1)), gate_steps=z(3))}),
    'conv3d_fwd': (lambda: dict(x=cl(*V), w_tck=z(27, 8, 4), bias=z(4), **C3), ['conv3d_fwd'], [((2, 4, 3, 4, 5), F32)],
                   {'filter channels': put('w_tck', lambda: z(27, 7, 4)), 'filter taps': put('w_tck', lambda: z(9, 8, 4)), 'bias short': short('bias'),
                    'out shape': put('out', lambda: cl(2, 4, 3, 4, 4)), 'residual short': put('residual', lambda: cl(1, 4, 3, 4, 5)), 'x dtype': to('x', F64)}),
    'conv3d_bwd_data': (lambda: dict(dy=cl(2, 4, 3, 4, 5), w_tkc=z(27, 4, 8), in_shape=V, **C3), ['conv3d_bwd_data'], [(V, F32)],
                        {'filter channels': put('w_tkc', lambda: z(27, 3, 8)), 'input size': put('in_shape', lambda: (2, 8, 3, 4, 6)), 'out shape': put('out', lambda: cl(2, 8, 3, 4, 4)),
                         'filter not dense': strided('w_tkc')}),
    'conv3d_bwd_weight': (lambda: dict(x=cl(*V), dy=cl(2, 4, 3, 4, 5), want_bias=True, **C3), ['conv3d_bwd_weight'], [((27, 8, 4), F32), ((4,), F32)],
                          {'dy short': short('dy'), 'out dw shape': put('out', lambda: (z(27, 8, 3), z(4))), 'out db missing': put('out', lambda: (z(27, 8, 4), None)),
                           'dy dtype': to('dy', F64)}),
    'groupnorm_relu_fwd': (lambda: dict(x=cl(*V), gamma=z(8), beta=z(8), G=2, eps=1e-5, relu=True), ['groupnorm_relu_fwd'], [(V, F32), ((2, 2), F32), ((2, 2), F32)],
                           {'gamma short': short('gamma'), 'beta short': short('beta'), 'beta dtype': to('beta', BF16), 'groups': put('G', lambda: 3)}),
    'groupnorm_relu_bwd': (lambda: dict(dy=cl(*V), x=cl(*V), gamma=z(8), beta=z(8), mean=z(2, 2), rstd=z(2, 2), G=2, relu=True), ['groupnorm_relu_bwd_add'],
                           [(V, F32), ((8,), F32), ((8,), F32)],
                           {'dy short': short('dy'), 'mean short': short('mean'), 'gamma short': short('gamma'), 'add short': put('add', lambda: cl(1, 8, 3, 4, 5)),
                            'rstd short': short('rstd'), 'rstd dtype': to('rstd', BF16)}),
    'upsample2x_add_fwd': (lambda: dict(x=cl(*V), skip=cl(2, 8, 6, 8, 10)), ['upsample2x_add_fwd'], [((2, 8, 6, 8, 10), F32)],
                           {'skip shape': put('skip', lambda: cl(2, 8, 6, 8, 9)), 'dtype': to('x', F64)}),
    'upsample2x_bwd': (lambda: dict(dy=cl(2, 8, 6, 8, 10)), ['upsample2x_bwd'], [(V, F32)], {'odd extent': put('dy', lambda: cl(2, 8, 5, 8, 10)), 'dtype': to('dy', F64)}),
    'cosine_top1': (lambda: dict(gallery=z(10, 16), gallery_label=z(10, dtype=I32), query=z(3, 16), query_label=z(3, dtype=I32)), ['cosine_top1'], [((3,), I32), ((3,), F32)],
                    {'gallery_label short': short('gallery_label'), 'query narrow': put('query', lambda: z(3, 15)), 'query_label dtype': to('query_label', I64),
                     'query on another device': meta('query'), 'gallery dtype': to('gallery', F64), 'gallery_label on another device': meta('gallery_label')}),
    'conv2d_2src_fwd': (lambda: dict(x=cl(*X4), s=cl(*X4), w_tck=z(9, 8, 4), bias=z(4), **CONV), ['conv2d_2src_fwd'], [(X4, F32)],
                        {'s short': short('s'), 'filter channels': put('w_tck', lambda: z(9, 7, 4)), 'bias short': short('bias'), 'out shape': put('out', lambda: cl(2, 4, 5, 5)),
                         'x bf16': to('x', BF16)}),
    'conv2d_2src_bwd_data': (lambda: dict(dy=cl(*X4), w_tkc=z(9, 4, 8), Cx=4, Cs=4, in_hw=(5, 6), **CONV), ['conv2d_2src_bwd_data'], [(X4, F32), (X4, F32)],
                             {'filter channels': put('w_tkc', lambda: z(9, 4, 7)), 'input size': put('in_hw', lambda: (6, 6)), 'ds_out shape': put('ds_out', lambda: cl(2, 4, 5, 5)),
                              'dx_out shape': put('dx_out', lambda: cl(2, 3, 5, 6))}),
    'conv2d_2src_bwd_weight': (lambda: dict(x=cl(*X4), s=cl(*X4), dy=cl(*X4), **CONV), ['conv2d_2src_bwd_weight'], [((9, 8, 4), F32), ((4,), F32)],
                               {'s short': short('s'), 'dy short': short('dy'), 'dw_out short': put('dw_out', lambda: z(9, 8, 3)), 'bias_sink short': put('bias_sink', lambda: z(3))}),
    'softplus_fwd': (lambda: dict(x=cl(*X4)), ['softplus_fwd'], [(X4, F32)], {'dtype': to('x', BF16), 'out shape': put('out', lambda: cl(2, 4, 5, 5))}),
    'softplus_bwd': (lambda: dict(dy=cl(*X4), x=cl(*X4)), ['softplus_bwd'], [(X4, F32)], {'dy short': short('dy'), 'dtype': to('dy', BF16), 'out shape': put('out', lambda: cl(2, 4, 5, 5))}),
    'softmax_fwd': (lambda: dict(s=cl(*X4)), ['softmax_fwd'], [(X4, F32)], {'dtype': to('s', BF16), 'out not NHWC': put('out', lambda: z(*X4))}),
    'softmax_bwd': (lambda: dict(dout=cl(*X4), out_fwd=cl(*X4)), ['softmax_bwd'], [(X4, F32)], {'dout short': short('dout'), 'out shape': put('out', lambda: cl(2, 4, 5, 5))}),
    'kl_fwd': (lambda: dict(mu_list=[z(2, 4), z(2, 4)], lv_list=[z(2, 4), z(2, 4)], weight=torch.ones(2, 2)), ['kl_fwd'], [((), F32)],
               {'weight narrow': put('weight', lambda: torch.ones(2, 1)), 'a block short': item('lv_list', 1, short), 'weight dtype': to('weight', F64),
                'prior shape': lambda kw: kw.update(pmu=z(2, 3), plv=z(2, 3)), 'half a prior': put('pmu', lambda: z(2, 4)), 'nine contrasts': lambda kw: kw.update(
                    mu_list=[z(2, 4)] * 9, lv_list=[z(2, 4)] * 9)}),
    'kl_bwd': (lambda: dict(dloss=torch.ones(()), mu_list=[z(2, 4), z(2, 4)], lv_list=[z(2, 4), z(2, 4)], weight=torch.ones(2, 2)), ['kl_bwd'], [((2, 2, 4), F32)] * 2,
               {'weight narrow': put('weight', lambda: torch.ones(2, 1)), 'a block short': item('mu_list', 1, short), 'two upstream gradients': put('dloss', lambda: z(2)),
                'a block dtype': item('lv_list', 0, lambda k: to(k, F64))}),
    'avgpool_fwd': (lambda: dict(x=cl(2, 8, 4, 6), k=2), ['avgpool_fwd'], [((2, 48), F32)], {'dtype': to('x', BF16), 'window': put('k', lambda: 0)}),
    'avgpool_bwd': (lambda: dict(dy=z(2, 48), in_shape=(2, 8, 4, 6), k=2), ['avgpool_bwd'], [((2, 8, 4, 6), F32)],
                    {'dy narrow': put('dy', lambda: z(2, 47)), 'dtype': to('dy', F64), 'out shape': put('out', lambda: cl(2, 8, 4, 5))}),
    'chatt_fwd': (lambda: dict(x=cl(*X), s=cl(*X), wd=z(2, 8), bd=z(2), wu=z(8, 2), bu=z(8)), ['chatt_fwd'], [(X, F32), ((2, 8), F32), ((2, 2), F32), ((2, 8), F32)],
                  {'s short': short('s'), 'W_down narrow': put('wd', lambda: z(2, 7)), 'b_up short': short('bu'), 'out shape': put('out', lambda: cl(2, 8, 5, 5)), 'W_up dtype': to('wu', F64)}),
    'chatt_bwd': (lambda: dict(dy=cl(*X), x=cl(*X), a=z(2, 8), hid=z(2, 2), pool=z(2, 8), wd=z(2, 8), wu=z(8, 2)), ['chatt_bwd'],
                  [(X, F32), ((2, 8), F32), ((2,), F32), ((8, 2), F32), ((8,), F32)],
                  {'a narrow': put('a', lambda: z(2, 7)), 'dy short': short('dy'), 'pool short': short('pool'), 'W_up shape': put('wu', lambda: z(8, 3))}),
    'symdiff_fwd': (lambda: dict(g=cl(*X4)), ['symdiff_fwd'], [(X4, F32)], {'dtype': to('g', BF16), 'out shape': put('out', lambda: cl(2, 4, 5, 5))}),
    'symdiff_bwd': (lambda: dict(dgd=cl(*X4), g=cl(*X4)), ['symdiff_bwd'], [(X4, F32)], {'dgd short': short('dgd'), 'out shape': put('out', lambda: cl(2, 4, 5, 5))}),
    'rgate_fwd': (lambda: dict(x=cl(2, 8, 4, 6), alpha=z(2, 1, 2, 3)), ['rgate_fwd'], [((2, 8, 4, 6), F32)],
                  {'alpha shape': put('alpha', lambda: z(2, 1, 2, 2)), 'alpha dtype': to('alpha', F64), 'out shape': put('out', lambda: cl(2, 8, 4, 5))}),
    'rgate_bwd': (lambda: dict(dy=cl(2, 8, 4, 6), x=cl(2, 8, 4, 6), alpha=z(2, 1, 2, 3)), ['rgate_bwd', 'bilinear_bwd'], [((2, 8, 4, 6), F32), ((2, 1, 2, 3), F32)],
                  {'dy short': short('dy'), 'alpha shape': put('alpha', lambda: z(2, 1, 2, 2))}),
}
DEVICE_ONLY = ('prep_stats', 'prep_write', 'export_volume')


def tensors(result):
    """the tensors of a wrapper's result, flattened in order"""
    if isinstance(result, torch.Tensor):
        return [result]
    if isinstance(result, (tuple, list)):
        return [t for r in result for t in tensors(r)]
    return []


def refusal_failures(stub):
    """every mutation of every row -> the ones that did NOT end in MrdisError before any compute entry point (explicit ifs: this also runs under python -O)"""
    failures, n = [], 0
    for name, (make, _, _, mutations) in sorted(ROWS.items()):
        for what, mutate in mutations.items():
            kw = make()
            mutate(kw)
            del stub.calls[:]
            n += 1
            try:
                getattr(hip, name)(**kw)
                how = 'no error'
            except hip.MrdisError:
                how = None
            except Exception as e:      # AssertionError, torch's RuntimeError, ctypes.ArgumentError, ... : not the refusal the binding promises
                how = f'{type(e).__name__}: {e}'
            if how is not None or stub.calls:
                failures.append(f'{name} [{what}]: {how or "MrdisError"}; entry points reached: {stub.calls}')
    return failures, n


def test_every_wrapper_has_a_row():
    """every public function of hip.py whose source names a compute entry point; a new wrapper fails here until it gets its row"""
    wrappers = set()
    for name, fn in vars(hip).items():
        if inspect.isfunction(fn) and fn.__module__ == hip.__name__ and not name.startswith('_'):
            if set(re.findall(r'\bmrdis_\w+', inspect.getsource(fn))) & COMPUTE:
                wrappers.add(name)
    assert len(wrappers) >= 80, sorted(wrappers)
    assert wrappers == set(ROWS), (sorted(wrappers - set(ROWS)), sorted(set(ROWS) - wrappers))
    for name, (make, calls, shapes, mutations) in ROWS.items():
        assert mutations, name
        assert (calls is None) == (name in DEVICE_ONLY), name      # the only rows without a valid-call half


def test_valid_calls_reach_their_entry_points(monkeypatch):
    stub = install_stub(monkeypatch.setattr)
    for name, (make, calls, shapes, _) in sorted(ROWS.items()):
        if name in DEVICE_ONLY:
            continue
        del stub.calls[:]
        result = getattr(hip, name)(**make())
        assert stub.calls == calls, (name, stub.calls, calls)
        got = [(tuple(t.shape), t.dtype) for t in tensors(result)]
        assert got == [(tuple(s), d) for s, d in shapes], (name, got, shapes)
        assert all(c in COMPUTE for c in ('mrdis_' + c for c in calls)), name


def test_mutated_calls_raise_before_any_entry_point(monkeypatch):
    stub = install_stub(monkeypatch.setattr)
    failures, n = refusal_failures(stub)
    assert n >= 250, n
    assert not failures, '\n'.join(failures)


def test_refusals_do_not_depend_on_assert():
    """the same refusals in a child `python -O`, which strips assert statements"""
    out = subprocess.run([sys.executable, '-O', os.path.abspath(__file__)], capture_output=True, text=True, timeout=300,
                         env={k: v for k, v in os.environ.items() if not k.startswith('MRDIS_')})
    assert out.returncode == 0 and 'refusals under -O: 0 failures' in out.stdout, out.stdout[-4000:] + out.stderr[-4000:]


if __name__ == '__main__':
    if __debug__:
        raise SystemExit('run with python -O')
    failures, n = refusal_failures(install_stub(setattr))
    print('\n'.join(failures))
    print(f'refusals under -O: {len(failures)} failures of {n}')
    raise SystemExit(1 if failures or n < 250 else 0)
