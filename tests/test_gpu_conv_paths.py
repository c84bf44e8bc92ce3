"""Every kernel the convolution dispatcher can reach (csrc/mrdis_conv.hip: mrdis_conv2d_fwd, _bwd_data, _bwd_weight, _fwd_spade), element by element
against float64 (tests/conv_check.py), with the launch counters proving which kernel produced the result.

One row = (entry point, storage, options, geometry) and the counted family it must launch; every other counted family must stay at 0.  Paths
without a counter (the tap-table direct kernel, the Cin = 4 / Cout = 4 / Cout = 16 fp32 kernels, the 1x1 head, the stride-2 first layers, the
generic and narrow weight-gradient kernels, the mixed-storage kernels) are rows whose expected set is empty: all counters 0 proves no counted
kernel took the call, and the row names how its own kernel is proved -- a different result from the next kernel of the dispatcher (`chain`), the
number of launches, the kernels a fresh process launches for the call alone (`lds_kernel`), no fallback (mixed storage), being the last kernel
(TERMINAL), or a stated reason (SAME_BITS).  Each row also runs on an input channel slice (ld > Ci) and writes into a channel slice of a wider
buffer prefilled with NaN: the neighbouring channels must still hold the same NaN bits afterwards.

kappa (tests/conv_check.py KAPPA): measured worst |got - ref| / (u A) per kernel and direction over all rows (profiles/conv_path_margins.txt,
recorded with MRDIS_DUMP_MEASURED=<dir>), times about 4.

The bf16 weight-gradient family (csrc/mrdis_bf16.hip: bwgrad_kernel, bwgrad2_kernel, bwgrad3_kernel, bwgrad_pack_kernel; counters 'bwgrad',
'bwgrad2', 'bwgrad3', 'bwgrad_s2') has one row per instantiation (BW_ROWS): the instantiation follows from (Ci, Co, storage) and stands in the
row id, the counter proves the kernel, tests/bwgrad_plan.py replays the planner for 256 CUs and says which (tiles, slabs) made it so.  Their kappa
is 4x the worst ratio of the same sums evaluated in plain fp32 on the CPU (tests/test_conv_check.py), not of the kernels.  The rows kept under
debug_mode 3010 (bwgrad2_kernel) must also equal the bwgrad3_kernel result of the same call bit for bit (`twin`)."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import conv_check as CC
from fixtures import dump_measured

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
B16 = torch.bfloat16
PAD_C = 8           # channels on each side of the input / output slices

# families of hip.KERNEL_FAMILIES that no row of this table launches, and why
NOT_IN_TABLE = {
    'all': 'every launch of the library, not a kernel',
    'zsearch': 'nearest-neighbour code search, not a convolution (tests/test_gpu_zsearch.py)',
    'wino_spade': '3-D only: counts mrdis_run_wino3d, the hybrid 3-D Winograd of mrdis_conv3d_fwd / _bwd_data, despite its name (tests/test_gpu_conv3d_paths.py)',
    'split6_c3d': '3-D only: mrdis_conv3d_s6.hip forward / data gradient, checked element-wise against float64 in tests/test_gpu_conv3d_paths.py',
    'split6_w3d': '3-D only: mrdis_conv3d_s6.hip weight gradient, checked element-wise against float64 in tests/test_gpu_conv3d_paths.py',
}

KAPPA = CC.KAPPA


def R(rid, op, geom, expect, opts=None, dtype='f32', img=None, lrelu=False, bias=True, sink=False, chain=None, kname=None, launches=None, lds_kernel=None,
      twin=None, fallback=False, in_pad=None):
    """geom = (N, Ci, Co, H, W, k, stride, pad); expect = the counted families that must launch (() for uncounted paths, then kname names the
    path); chain = options under which the next kernel of the dispatcher takes the call (its result must differ); launches = the number of
    library launches the call makes; lds_kernel = a kernel that must be among those a fresh process launches for this call alone (hip.dynamic_lds
    names the kernels launched with dynamic LDS; the tap-table kernel must not be among them); dtype: 'f32' | 'bf16' | one of MIXED | 'bf16m'
    (weight gradients: fp32 views, MRDIS_DT_F32_BF16M); twin = (options, family): the same call under these options must launch that other family
    and return the same bits; fallback: hip.fallbacks['conv2d_bwd_weight_bf16'] must rise by one during the row (the bf16 kernels declined and
    the fp32 kernels ran between two view casts); in_pad = (left, right) channels around the input slices instead of (PAD_C, PAD_C)"""
    return pytest.param(dict(op=op, geom=geom, expect=tuple(expect), opts=opts or {}, dtype=dtype, img=img, lrelu=lrelu, bias=bias, sink=sink,
                             chain=chain, kname=kname or expect[0], launches=launches, lds_kernel=lds_kernel, twin=twin, fallback=fallback,
                             in_pad=in_pad), id=rid)


W2 = {'wino': 2}                       # Winograd wherever it applies (the size policy takes these kernels only on big grids)
NOW16 = {'debug_now16': 1}             # turns off the 1x1 head, the Cout = 16 forward, the stride-2 first-layer and the narrow weight-gradient kernels
# uncounted rows without a chain: the last kernel of the dispatcher's order for their call (nothing after it to compare with), where all counters
# at 0 and no declining kernel before it is the proof
TERMINAL = {'direct': 'the tap-table direct kernel (run_tapconv)', 'direct_s2': 'the tap-table kernel on the four stride-2 parity classes',
            'wgrad': 'the generic weight-gradient kernel (plan_wgrad)', 'bconv': 'the generic bf16 tap kernel'}
# uncounted rows whose kernel computes the same bits as the next one and launches no kernel with dynamic LDS (so lds_kernel cannot name it)
SAME_BITS = {'pw dgrad': 'the <= 8 products of a 1x1 data gradient are summed in the same order by the generic kernel; all counters 0 is the proof'}
MIXED = ('xb_yf', 'xf_yb')             # bf16 x / fp32 y and fp32 x / bf16 y (MRDIS_DT_XBF16_YF32 / _XF32_YBF16)
ROWS = [
    # ---- F(2x2) phase-by-phase (mrdis_wino.hip): 32- and 64-cout variants; forward and the flipped-filter data gradient
    R('wino fwd 1x1 map', 'fwd', (1, 16, 32, 1, 1, 3, 1, 1), ['wino'], {**W2, 'wino_pipe': 0}),
    R('wino fwd 2x3 cin/cout tails', 'fwd', (2, 24, 40, 2, 3, 3, 1, 1), ['wino'], {**W2, 'wino_pipe': 0}, lrelu=True),
    R('wino fwd odd ragged 64-cout', 'fwd', (3, 40, 72, 17, 23, 3, 1, 1), ['wino'], {**W2, 'wino_pipe': 0}, bias=False),
    R('wino dgrad', 'dgrad', (2, 24, 40, 9, 7, 3, 1, 1), ['wino'], {**W2, 'wino_pipe': 0}),
    # ---- F(2x2) pipelined (mrdis_wino2.hip, Cout > 32)
    R('wino2 fwd 3x2', 'fwd', (1, 8, 40, 3, 2, 3, 1, 1), ['wino2'], W2, lrelu=True),
    R('wino2 fwd persistent walk', 'fwd', (8, 36, 72, 33, 35, 3, 1, 1), ['wino2'], W2),
    R('wino2 dgrad', 'dgrad', (2, 72, 36, 11, 13, 3, 1, 1), ['wino2'], W2),
    # ---- F(4x4) (mrdis_wino4.hip: filter image format 4), narrow (format 5: wino4n / register-fed wino4r)
    R('wino4 fwd', 'fwd', (2, 64, 64, 20, 37, 3, 1, 1), ['wino4'], {**W2, 'wino4': 2}, img='wino', lrelu=True),
    R('wino4 fwd cin/cout tails', 'fwd', (2, 16, 72, 33, 31, 3, 1, 1), ['wino4'], {**W2, 'wino4': 2}, img='wino'),
    R('wino4 dgrad', 'dgrad', (1, 72, 96, 11, 21, 3, 1, 1), ['wino4'], {**W2, 'wino4': 2}, img='wino'),
    R('wino4n fwd', 'fwd', (3, 72, 20, 19, 27, 3, 1, 1), ['wino4n'], {**W2, 'wino4': 2, 'wino4r': 0}, img='wino', lrelu=True),
    R('wino4r fwd 64-tile', 'fwd', (1, 24, 32, 17, 96, 3, 1, 1), ['wino4r'], {**W2, 'wino4': 2, 'wino4r': 2}, img='wino'),
    R('wino4r fwd channel split', 'fwd', (2, 64, 32, 17, 37, 3, 1, 1), ['wino4r'], {**W2, 'wino4': 2, 'wino4r': 3}, img='wino'),
    # ---- Winograd weight gradients
    R('wino_wgrad 64x32 blocks', 'wgrad', (2, 64, 32, 22, 30, 3, 1, 1), ['wino_wgrad'], {**W2, 'wino4': 0, 'wino_pipe': 0}),
    R('wino_wgrad 32x64 blocks odd', 'wgrad', (2, 32, 64, 17, 21, 3, 1, 1), ['wino_wgrad'], {**W2, 'wino4': 0}, sink=True),
    R('wino_wgrad2', 'wgrad', (3, 64, 128, 7, 5, 3, 1, 1), ['wino_wgrad2'], {**W2, 'wino4': 0}),
    R('wino_wgrad2 1x1 map', 'wgrad', (2, 64, 64, 1, 1, 3, 1, 1), ['wino_wgrad2'], {**W2, 'wino4': 0}, sink=True),
    R('wino4_wgrad', 'wgrad', (2, 32, 64, 8, 16, 3, 1, 1), ['wino4_wgrad'], {**W2, 'wino4': 2}),
    R('wino4_wgrad several blocks', 'wgrad', (3, 64, 128, 16, 8, 3, 1, 1), ['wino4_wgrad'], {**W2, 'wino4': 2}, sink=True),
    # ---- fused gamma | beta + SPADE modulation
    R('wino2_spade', 'spade', (2, 32, 48, 24, 40, 3, 1, 1), ['wino2_spade'], W2),
    R('wino4_spade', 'spade', (3, 64, 64, 50, 72, 3, 1, 1), ['wino4_spade'], {**W2, 'wino4': 2}, img='wino'),
    # ---- bf16 activations (MRDIS_DT_BF16): bconv3 (mrdis_bf16p.hip) / bconv4 (mrdis_bf16q.hip, LDS-DMA)
    R('bconv3 fwd ragged', 'fwd', (2, 32, 40, 23, 37, 3, 1, 1), ['bconv3'], {'bconv4': 0}, dtype='bf16', lrelu=True),
    R('bconv3 fwd 16 couts narrow map', 'fwd', (1, 96, 16, 9, 70, 3, 1, 1), ['bconv3'], {'bconv4': 0}, dtype='bf16'),
    R('bconv3 dgrad', 'dgrad', (2, 32, 64, 23, 37, 3, 1, 1), ['bconv3'], {'bconv4': 0}, dtype='bf16'),
    R('bconv4 fwd ragged', 'fwd', (2, 32, 40, 23, 37, 3, 1, 1), ['bconv4'], {'bconv4': 2}, dtype='bf16', lrelu=True),
    R('bconv4 fwd 32-cout instantiation', 'fwd', (9, 32, 16, 48, 64, 3, 1, 1), ['bconv4'], {'bconv4': 2}, dtype='bf16'),
    R('bconv4 fwd cout tail 72', 'fwd', (5, 32, 72, 16, 33, 3, 1, 1), ['bconv4'], {'bconv4': 2}, dtype='bf16', bias=False),
    R('bconv4 dgrad', 'dgrad', (2, 32, 64, 23, 37, 3, 1, 1), ['bconv4'], {'bconv4': 2}, dtype='bf16'),
    R('bconv4 dgrad 96 reduce', 'dgrad', (1, 64, 96, 17, 40, 3, 1, 1), ['bconv4'], {'bconv4': 2}, dtype='bf16'),
    R('bconv3_spade', 'spade', (2, 32, 48, 20, 33, 3, 1, 1), ['bconv3_spade'], {'bconv4': 0}, dtype='bf16'),
    R('bconv4_spade', 'spade', (4, 32, 16, 16, 32, 3, 1, 1), ['bconv4_spade'], {'bconv4': 2}, dtype='bf16'),
    R('bconv4_spade ragged', 'spade', (3, 64, 64, 21, 47, 3, 1, 1), ['bconv4_spade'], {'bconv4': 2}, dtype='bf16'),
    R('bconv generic (bf16 stride 2)', 'fwd', (2, 32, 64, 16, 24, 4, 2, 1), [], dtype='bf16', kname='bconv'),
    # bf16 views the bf16 weight-gradient family declines: hip.conv2d_bwd_weight runs the fp32 generic kernel between two view casts and counts
    # the fallback.  1702 positions (plan_bwgrad wants 4096); a pixel stride of Ci + 12 channels (run_bwgrad wants a multiple of 8) at the
    # 4096-position geometry that the family otherwise takes ('bwgrad<1,2,__bf16> 4096 positions' below); stride 2 with the family switched off
    R('wgrad bf16 tiny-map fallback', 'wgrad', (2, 32, 64, 23, 37, 3, 1, 1), [], dtype='bf16', sink=True, kname='wgrad', fallback=True),
    R('wgrad bf16 fallback pixel stride % 8 != 0', 'wgrad', (1, 32, 64, 64, 64, 3, 1, 1), [], {'wino': 0}, dtype='bf16', kname='wgrad', fallback=True, in_pad=(8, 4)),
    R('wgrad bf16 s2 fallback (debug_now16)', 'wgrad', (8, 32, 24, 34, 38, 3, 2, 1), [], NOW16, dtype='bf16', sink=True, kname='wgrad', fallback=True),
    # ---- six-product kernels (option split6)
    R('split6_c4 fwd', 'fwd', (2, 4, 32, 3, 5, 3, 1, 1), ['split6_c4'], {'split6': 1}, lrelu=True),
    R('split6_c4 fwd cout tail', 'fwd', (1, 4, 20, 33, 47, 3, 1, 1), ['split6_c4'], {'split6': 1}),
    R('split6_co4 fwd', 'fwd', (16, 32, 4, 65, 64, 3, 1, 1), ['split6_co4'], {'split6': 1}, lrelu=True),
    R('split6_co4 dgrad (4 <- 64)', 'dgrad', (8, 4, 64, 33, 256, 3, 1, 1), ['split6_co4'], {'split6': 1}),
    R('split6_c16 fwd', 'fwd', (1, 32, 16, 257, 256, 3, 1, 1), ['split6_c16'], {'split6': 1}, lrelu=True),
    R('split6_wgrad16', 'wgrad', (2, 32, 16, 225, 230, 3, 1, 1), ['split6_wgrad16'], {'split6': 1}, sink=True),
    R('split6_tap fwd s1', 'fwd', (5, 24, 20, 19, 23, 3, 1, 1), ['split6_tap'], {'split6': 10}, img='s6', lrelu=True),
    R('split6_tap fwd s2', 'fwd', (3, 40, 36, 22, 26, 4, 2, 1), ['split6_tap'], {'split6': 10}, img='s6'),
    R('split6_tap dgrad s2', 'dgrad', (3, 40, 32, 22, 26, 4, 2, 1), ['split6_tap'], {'split6': 10}, img='s6'),
    # ---- paths without a counter: all counters 0, and (chain) a different result from the counted kernel the defaults would pick
    R('direct fwd odd', 'fwd', (1, 5, 6, 9, 11, 3, 1, 1), [], {'wino': 0}, kname='direct', lrelu=True),
    R('direct fwd 1x2 map', 'fwd', (2, 96, 40, 1, 2, 3, 1, 1), [], {'wino': 0}, kname='direct', chain=W2),
    R('direct fwd s2 4x4', 'fwd', (2, 64, 72, 10, 13, 4, 2, 1), [], kname='direct'),
    R('direct fwd 3x3 map split-k', 'fwd', (1, 256, 48, 3, 3, 3, 1, 1), [], {'wino': 0}, kname='direct', chain=W2),
    R('direct dgrad', 'dgrad', (2, 40, 72, 7, 9, 3, 1, 1), [], {'wino': 0}, kname='direct', chain=W2),
    R('direct dgrad s2 packed', 'dgrad', (2, 32, 64, 16, 24, 4, 2, 1), [], kname='direct_s2', launches=1),       # four parity classes, one launch
    R('direct dgrad s2 four launches', 'dgrad', (2, 32, 64, 15, 23, 4, 2, 1), [], {'debug_nopack': 1}, kname='direct_s2', launches=4),
    R('direct dgrad s2 3x3 odd', 'dgrad', (3, 16, 24, 11, 13, 3, 2, 1), [], kname='direct_s2'),
    R('c4 fp32 fwd', 'fwd', (2, 4, 32, 9, 33, 3, 1, 1), [], {'split6': 0}, kname='c4', lrelu=True, chain={'split6': 1}),
    R('c4 fp32 fwd 64 couts', 'fwd', (1, 4, 64, 2, 3, 3, 1, 1), [], {'split6': 0}, kname='c4', chain={'split6': 4}),
    R('co4 fp32 fwd', 'fwd', (16, 32, 4, 65, 64, 3, 1, 1), [], {'split6': 0}, kname='co4', chain={'split6': 1}),
    R('co4 fp32 dgrad', 'dgrad', (8, 4, 64, 33, 256, 3, 1, 1), [], {'split6': 0}, kname='co4', chain={'split6': 1}),
    R('c16 fp32 fwd 32 -> 16', 'fwd', (1, 32, 16, 257, 256, 3, 1, 1), [], {'split6': 0}, kname='c16', chain={'split6': 1}),
    R('c16 fp32 fwd 16 -> 16', 'fwd', (1, 16, 16, 256, 257, 3, 1, 1), [], kname='c16', lrelu=True, chain=NOW16),
    R('pw fwd 1x1 head', 'fwd', (2, 16, 7, 64, 48, 1, 1, 0), [], kname='pw', chain=NOW16),
    R('pw fwd generic', 'fwd', (2, 16, 7, 64, 48, 1, 1, 0), [], NOW16, kname='direct'),
    R('pw dgrad', 'dgrad', (2, 16, 7, 64, 65, 1, 1, 0), [], kname='pw'),      # see SAME_BITS
    R('pw wgrad', 'wgrad', (2, 16, 7, 64, 48, 1, 1, 0), [], kname='pw', sink=True, chain=NOW16),
    # stride-2 first layers (mrdis_wgrad_s2.hip): Cin <= 7, Cout 16 | 32, even H, W % 32 == 0 (data gradient: W 128 | 256), >= 100000 pixels
    # (the forward computes the same bits as the tap-table kernel: proved by the kernels a fresh process launches for this call alone)
    R('s2 fwd first layer 4x4', 'fwd', (2, 7, 16, 256, 256, 4, 2, 1), [], kname='s2', lrelu=True, lds_kernel='conv_s2_fwd_kernel'),
    R('s2 fwd 3x3 odd cin', 'fwd', (7, 3, 32, 112, 128, 3, 2, 1), [], kname='s2', lds_kernel='conv_s2_fwd_kernel'),
    R('s2 dgrad 4x4', 'dgrad', (7, 4, 32, 112, 128, 4, 2, 1), [], kname='s2', chain=NOW16),
    R('s2 dgrad 3x3', 'dgrad', (2, 7, 16, 256, 256, 3, 2, 1), [], kname='s2', chain=NOW16),
    R('wgrad generic', 'wgrad', (2, 96, 40, 20, 24, 3, 1, 1), [], {'wino': 0}, kname='wgrad'),
    R('wgrad generic 1x1 map', 'wgrad', (2, 24, 20, 1, 1, 3, 1, 1), [], {'wino': 0}, kname='wgrad', sink=True),
    R('wgrad generic s2', 'wgrad', (2, 32, 64, 16, 24, 4, 2, 1), [], kname='wgrad'),
    R('wgrad_s2 first layer 4x4', 'wgrad', (2, 7, 32, 256, 256, 4, 2, 1), [], kname='wgrad_s2', chain=NOW16),
    R('wgrad_s2 3x3', 'wgrad', (7, 3, 16, 112, 128, 3, 2, 1), [], kname='wgrad_s2', sink=True, chain=NOW16),
    # narrow weight gradients: wgrad16 (Cout 8 | 12 | 16, Cin % 16 == 0), wgrad_c4 (Cin = 4, W 64 | 128 | 256), both >= 100000 pixels
    R('wgrad16 fp32', 'wgrad', (2, 32, 16, 225, 230, 3, 1, 1), [], {'split6': 0}, kname='wgrad16', chain=NOW16),
    R('wgrad16 fp32 8 couts', 'wgrad', (1, 16, 8, 320, 317, 3, 1, 1), [], kname='wgrad16', sink=True, chain=NOW16),
    R('wgrad_c4', 'wgrad', (2, 4, 32, 201, 256, 3, 1, 1), [], kname='wgrad_c4', sink=True, chain=NOW16),
    R('wgrad_c4 64 couts', 'wgrad', (13, 4, 64, 121, 64, 3, 1, 1), [], kname='wgrad_c4', chain=NOW16),
    R('wgrad16 bf16', 'wgrad', (2, 32, 16, 225, 230, 3, 1, 1), [], dtype='bf16', kname='wgrad16_bf16', sink=True, chain={'debug_mode': 3030}),
    # mixed storage (one bf16 side): these calls have no fallback -- a declined geometry is an error, so reaching the kernel is proved by the call
    R('pw head fwd bf16 x -> fp32 y', 'fwd', (2, 16, 7, 64, 48, 1, 1, 0), [], dtype='xb_yf', kname='pw_mixed'),
    R('pw head dgrad fp32 dy -> bf16 dx', 'dgrad', (2, 16, 7, 33, 35, 1, 1, 0), [], dtype='xb_yf', kname='pw_mixed'),
    R('pw head wgrad bf16 x, fp32 dy', 'wgrad', (2, 16, 7, 64, 48, 1, 1, 0), [], dtype='xb_yf', kname='pw_mixed', sink=True),
    R('co4 fwd bf16 x -> fp32 y (C -> 4)', 'fwd', (16, 32, 4, 65, 64, 3, 1, 1), [], dtype='xb_yf', kname='co4_mixed'),
    R('c4 dgrad fp32 dy -> bf16 dx (C <- 4)', 'dgrad', (2, 32, 4, 9, 33, 3, 1, 1), [], dtype='xb_yf', kname='c4_mixed'),
    R('wgrad_co4b bf16 x, fp32 dy (C -> 4)', 'wgrad', (2, 32, 4, 200, 256, 3, 1, 1), [], dtype='xb_yf', kname='wgrad_co4b', sink=True),
    R('c4 fwd fp32 x -> bf16 y (4 -> C)', 'fwd', (2, 4, 32, 9, 33, 3, 1, 1), [], dtype='xf_yb', kname='c4_mixed'),
    R('co4 dgrad bf16 dy -> fp32 dx (4 <- C)', 'dgrad', (16, 4, 32, 65, 64, 3, 1, 1), [], dtype='xf_yb', kname='co4_mixed'),
    R('wgrad_c4 fp32 x, bf16 dy (4 -> C)', 'wgrad', (2, 4, 32, 200, 256, 3, 1, 1), [], dtype='xf_yb', kname='wgrad_c4_mixed'),
]

# ---- the bf16 weight-gradient family (csrc/mrdis_bf16.hip).  Every row is a wgrad row with need_bias on channel slices, alternately with and
# without a bias sink, and expects exactly one of 'bwgrad' | 'bwgrad2' | 'bwgrad3' | 'bwgrad_s2'.  The instantiation <WCI,WCO[,TS][,HALF]> in the id
# follows from the channels: WCI = 2 iff Ci % 64 == 0, WCO = 2 iff Co > 32, HALF iff Ci = 16, TS = float for 'bf16m' (fp32 views).
# tiles / slabs: what plan_bwgrad gives on 256 CUs (tests/bwgrad_plan.py; tests/test_conv_check.py holds these rows to it): bwgrad3_kernel needs
# tiles >= 3 slabs, bwgrad2_kernel tiles >= 2 slabs.  The slab count is also what bwgrad_reduce_kernel walks: its wave w sums the slabs w, w + 16,
# ... four at a time while k + 48 < slabs, then one at a time -- <= 16 slabs: at most one per wave; 17 .. 48: the tail loop alone; >= 65: the
# unrolled body and the tail in the same wave.
BW3 = {         # 3x3 stride 1 pad 1, bf16 views, defaults -> bwgrad3_kernel; (N, Ci, Co, H, W)
    '<1,1> ragged in H and W': (5, 96, 16, 129, 33),             # 330 tiles / 86 slabs (reduce: unrolled body + tail); the last tile row holds 1 of 4 rows, the last column 1 of 32
    '<1,2> cout tail 72 of 128': (2, 96, 72, 129, 33),           # 132 / 43 (reduce: tail loop alone)
    '<2,1>': (3, 256, 16, 129, 33),                              # 198 / 64
    '<2,2>': (3, 128, 72, 129, 33),                              # 198 / 64
    '<2,2> many-image tiles': (193, 128, 256, 8, 8),             # 97 / 32; NB = 2 images per tile, the last tile has one
    '<2,2> tiles narrower than 32': (25, 128, 256, 33, 15),      # 125 / 32; TW = 16, TH = 8
    '<2,2> 16 slabs': (2, 256, 256, 65, 33),                     # 68 / 16 (reduce: one slab per wave)
}
M3010 = {'debug_mode': 3010}           # keeps bwgrad2_kernel where bwgrad3_kernel would run
S2 = {          # stride 2 pad 1, bf16 views -> bwgrad_pack_kernel, the four parity classes in one launch; (N, Ci, Co, H, W, k)
    '<1,1,false> 3x3': (8, 32, 24, 34, 38, 3),                   # 40 tiles / 40 slabs per class; 17 x 19 class maps
    '<1,2,false> 4x4': (8, 96, 40, 34, 38, 4),                   # 40 / 22
    '<2,1,false> 3x3': (8, 64, 32, 36, 60, 3),                   # 40 / 40; 18 x 30 class maps
    '<2,2,false> 4x4': (6, 64, 40, 52, 76, 4),                   # 84 / 64; 26 x 38 class maps
    '<1,1,HALF> 3x3': (16, 16, 32, 32, 48, 3),                   # 64 / 64
    '<1,2,HALF> 4x4': (8, 16, 40, 34, 38, 4),                    # 40 / 40
}


def _bw_rows():
    rows = []

    def add(rid, shape, fam, opts=None, dtype='bf16', k=3, st=1, twin=None):
        rows.append(R(rid, 'wgrad', tuple(shape) + (k, st, 1), [fam], opts, dtype=dtype, sink=len(rows) % 2 == 0, twin=twin, launches=2))       # the kernel + the reduce
    for name, shape in BW3.items():
        add(f'bwgrad3{name}', shape, 'bwgrad3')
    for name, shape in BW3.items():        # the same calls on bwgrad2_kernel: the result must be the bwgrad3_kernel one bit for bit
        add(f'bwgrad2{name} (debug_mode 3010)', shape, 'bwgrad2', M3010, twin=({'debug_mode': -1}, 'bwgrad3'))
    add('bwgrad2<1,1> natural window', (3, 96, 16, 129, 33), 'bwgrad2')                     # 198 / 86: 2 slabs <= tiles < 3 slabs, defaults
    add('bwgrad<1,2,__bf16> cout tail 72 (wino_pipe 0)', BW3['<1,2> cout tail 72 of 128'], 'bwgrad', {'wino_pipe': 0})      # 132 / 43
    add('bwgrad<2,1,__bf16> (wino_pipe 0)', BW3['<2,1>'], 'bwgrad', {'wino_pipe': 0})                                       # 198 / 64
    # small grids, defaults: tiles = slabs (one tile per workgroup), so neither pipelined form applies
    add('bwgrad<1,1,__bf16>', (1, 32, 16, 65, 65), 'bwgrad')                                # 51 / 51 (reduce: the unrolled body in waves 0 .. 2 only)
    add('bwgrad<1,2,__bf16> cout tail 40', (1, 32, 40, 65, 65), 'bwgrad')                   # 51 / 51
    add('bwgrad<2,1,__bf16>', (1, 64, 16, 65, 65), 'bwgrad')                                # 51 / 51
    add('bwgrad<2,2,__bf16> cout tail 40', (1, 64, 40, 65, 65), 'bwgrad')                   # 51 / 51
    add('bwgrad<1,1,__bf16,HALF>', (1, 16, 24, 65, 65), 'bwgrad')                           # 51 / 51
    add('bwgrad<1,2,__bf16,HALF>', (1, 16, 40, 65, 65), 'bwgrad')                           # 51 / 51
    add('bwgrad<1,2,__bf16> 4096 positions', (1, 32, 64, 64, 64), 'bwgrad')                 # 32 / 32: the smallest map plan_bwgrad takes
    add('bwgrad<1,2,__bf16> many-image tiles', (64, 32, 64, 8, 8), 'bwgrad')                # 32 / 32; NB = 2
    # fp32 views, bf16 MFMA operands (MRDIS_DT_F32_BF16M; taken for Co > 32 or Ci >= 128)
    add('bwgrad<1,2,float>', (1, 32, 40, 65, 65), 'bwgrad', dtype='bf16m')                  # 51 / 51
    add('bwgrad<2,2,float>', (1, 64, 72, 65, 67), 'bwgrad', dtype='bf16m')                  # 51 / 51
    add('bwgrad<2,1,float>', (1, 128, 16, 65, 65), 'bwgrad', dtype='bf16m')                 # 51 / 51
    add('bwgrad<1,2,float> 96 cin', (1, 96, 40, 33, 130), 'bwgrad', dtype='bf16m')          # 45 / 45
    add('bwgrad<1,1,float> 160 cin', (1, 160, 16, 65, 65), 'bwgrad', dtype='bf16m')         # 51 / 51; Co <= 32 needs Ci >= 128, WCI = 1 needs Ci % 64 != 0
    for name, shape in S2.items():
        add(f'bwgrad_s2{name}', shape[:5], 'bwgrad_s2', k=shape[5], st=2)
    return rows


BW_ROWS = _bw_rows()
ROWS += BW_ROWS


@pytest.fixture(autouse=True)
def _cpu_threads():
    """the float64 references on at most 16 CPU threads"""
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    yield
    torch.set_num_threads(n)


def rnd(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def tck(w):
    return w.permute(2, 3, 1, 0).reshape(-1, w.shape[1], w.shape[0]).contiguous().to(DEV)


def tkc(w):
    return w.permute(2, 3, 0, 1).reshape(-1, w.shape[0], w.shape[1]).contiguous().to(DEV)


def in_slice(t, dtype, seed, pad=None):
    """t (N, C, H, W) as a channel slice (ld = C + 2 PAD_C; C + left + right for pad = (left, right)) of a wider NHWC device buffer"""
    N, C, H, W = t.shape
    left, right = pad or (PAD_C, PAD_C)
    wide = torch.cat([rnd((N, left, H, W), seed), t, rnd((N, right, H, W), seed + 1)], 1)
    wide = wide.to(DEV).contiguous(memory_format=torch.channels_last).to(dtype)
    return wide[:, left:left + C]


def out_slice(N, C, H, W, dtype):
    """(buffer of C + 2 PAD_C channels prefilled with NaN, the channel slice to write)"""
    buf = torch.empty((N, C + 2 * PAD_C, H, W), dtype=dtype, device=DEV, memory_format=torch.channels_last).fill_(float('nan'))
    return buf, buf[:, PAD_C:PAD_C + C]


def assert_neighbours_untouched(buf, C, what):
    it = torch.int32 if buf.dtype is torch.float32 else torch.int16
    nan = torch.full((1,), float('nan'), dtype=buf.dtype).view(it).item()
    for side in (buf[:, :PAD_C], buf[:, PAD_C + C:]):
        bits = side.contiguous().view(it)
        assert bool((bits == nan).all()), f'{what}: a store landed outside the output channel slice'


def wino_image(hip, w, R_, S, flip, spadeC=0):
    img = torch.full((hip.wino_u_image_floats(R_, S, spadeC),), float('nan'), device=DEV)
    j = hip.WinoUJob(); j.w, j.img, j.R, j.S, j.flip, j.spadeC, j.block0, j.nblk = w.data_ptr(), img.data_ptr(), R_, S, flip, spadeC, 0, hip.wino_u_job_blocks(R_, S, spadeC)
    hip.wino_u_jobs(hip.wino_u_table([j], DEV), 1, j.nblk)
    assert torch.isfinite(img).all()
    return img


@functools.lru_cache(maxsize=4)
def wgrad_operands(geom, dtype, seed=0):
    """the operands of a weight-gradient row and its float64 reference -> (x, dy, ref_w, A_w, ref_b, A_b); shared by the rows of one geometry, by a
    row and its twin, and by tests/test_conv_check.py: treat as read-only.  dw is referred to the values the kernel multiplies (bf16-rounded for
    bf16 views and for 'bf16m'), the bias to the values it sums: the view's own, so for 'bf16m' the fp32 dy before the rounding"""
    N, Ci, Co, H, W, k, st, pad = geom
    Ho, Wo = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
    x, dy = rnd((N, Ci, H, W), 1 + seed), rnd((N, Co, Ho, Wo), 4 + seed)
    x_in = CC.bf16_round if dtype in ('bf16', 'xb_yf', 'bf16m') else (lambda t: t.double())
    y_in = CC.bf16_round if dtype in ('bf16', 'xf_yb', 'bf16m') else (lambda t: t.double())
    ref_w, A_w, ref_b, A_b = CC.wgrad_ref(x_in(x), y_in(dy), k, k, st, pad)
    if dtype == 'bf16m':
        ref_b, A_b = dy.double().sum((0, 2, 3)), dy.double().abs().sum((0, 2, 3))
    return x, dy, ref_w, A_w, ref_b, A_b


def wgrad_yardstick(row, seed=0):
    """{'dw': ratio, 'db': ratio} of the row's sums evaluated in plain fp32 by torch on the CPU (CC.wgrad_fp32) against the row's float64
    reference: the rounding error that any fp32 accumulation of these sums carries, which the row's kappa is 4x of"""
    x, dy, ref_w, A_w, ref_b, A_b = wgrad_operands(row['geom'], row['dtype'], seed)
    k, st, pad = row['geom'][5:]
    dw, db = CC.wgrad_fp32(x, dy, k, st, pad, rounded_bias=row['dtype'] != 'bf16m')
    return {'dw': CC.ratio(dw, ref_w, A_w), 'db': CC.ratio(db, ref_b, A_b)}


def counted(hip):
    """the launch counters since the last reset ('all': every launch of the library)"""
    return {f: n for f, n in hip.launch_counts(reset=True).items() if f != 'zsearch'}


def run_row(hip, row, seed=0):
    """-> (results {name: (got, ref, A, u_out, extra)}, counts, the raw primary output for the chain comparison)"""
    N, Ci, Co, H, W, k, st, pad = row['geom']
    Ho, Wo = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
    op, dtype = row['op'], row['dtype']
    bf = dtype == 'bf16'
    xdt = B16 if dtype in ('bf16', 'xb_yf') else torch.float32          # the input-side view (x, dx)
    ydt = B16 if dtype in ('bf16', 'xf_yb') else torch.float32          # the output-side view (y, dy)
    x_in = CC.bf16_round if xdt is B16 else (lambda t: t.double())
    y_in = CC.bf16_round if ydt is B16 else (lambda t: t.double())
    w_in = CC.bf16_round if bf else (lambda t: t.double())              # (the mixed-storage kernels read the fp32 filter)
    u_y = CC.U_BF16 if ydt is B16 else 0.0
    u_x = CC.U_BF16 if xdt is B16 else 0.0
    if op == 'wgrad':
        x, dy, ref_w, A_w, ref_b, A_b = wgrad_operands(row['geom'], dtype, seed)
    else:
        x = rnd((N, Ci, H, W), 1 + seed)
        dy = rnd((N, Co, Ho, Wo), 4 + seed)
    w = rnd((Co, Ci, k, k), 2 + seed, (Ci * k * k) ** -0.5)
    b = rnd((Co,), 3 + seed, 0.1) if row['bias'] else None
    wt, wk = tck(w), tkc(w)
    if dtype in MIXED and k == 3 and 4 in (Ci, Co):      # the 3x3 layers with a four-channel side take the filter with that side padded to 16 (zeros)
        T = k * k
        if Ci == 4:
            wt = torch.cat([wt, torch.zeros(T, 12, Co, device=DEV)], 1); wk = torch.cat([wk, torch.zeros(T, Co, 12, device=DEV)], 2)
        else:
            wt = torch.cat([wt, torch.zeros(T, Ci, 12, device=DEV)], 2); wk = torch.cat([wk, torch.zeros(T, 12, Ci, device=DEV)], 1)
    res = {}
    hip.launch_counts(reset=True)
    if op == 'fwd':
        img = None
        if row['img'] == 'wino':
            img = wino_image(hip, wt, Ci, Co, 0)
        elif row['img'] == 's6':
            img = hip.s6_filter_image(wt)
        hip.launch_counts(reset=True)
        buf, out = out_slice(N, Co, Ho, Wo, ydt)
        hip.conv2d_fwd(in_slice(x, xdt, 11), wt, None if b is None else b.to(DEV), k, k, st, pad, lrelu=row['lrelu'], out=out,
                       w_bf16=hip.cast_bf16(wk) if bf else None, w_wino=img)
        c = counted(hip)
        assert_neighbours_untouched(buf, Co, 'fwd')
        ref, A = CC.fwd_ref(x_in(x), w_in(w), b, st, pad, row['lrelu'])
        res['y'] = (out, ref, A, u_y, None)
        prim = out
    elif op == 'dgrad':
        img = None
        if row['img'] == 'wino':
            img = wino_image(hip, wk, Co, Ci, 1)
        elif row['img'] == 's6':
            img = hip.s6_filter_image(wk)
        hip.launch_counts(reset=True)
        buf, out = out_slice(N, Ci, H, W, xdt)
        hip.conv2d_bwd_data(in_slice(dy, ydt, 13), wk, (H, W), k, k, st, pad, w_bf16=hip.cast_bf16(wt) if bf else None, out=out, w_wino=img)
        c = counted(hip)
        assert_neighbours_untouched(buf, Ci, 'dgrad')
        ref, A = CC.dgrad_ref(y_in(dy), w_in(w), (H, W), st, pad)
        res['dx'] = (out, ref, A, u_x, None)
        prim = out
    elif op == 'wgrad':
        s0 = rnd((Co,), 5 + seed)
        sink = s0.to(DEV) if row['sink'] else None
        dw, db = hip.conv2d_bwd_weight(in_slice(x, xdt, 11, row['in_pad']), in_slice(dy, ydt, 13, row['in_pad']), k, k, st, pad, need_bias=True, bias_sink=sink,
                                       dtype=hip.DT_F32_BF16M if dtype == 'bf16m' else hip.DT_F32)
        c = counted(hip)
        got_w = dw.reshape(k, k, Ci, Co).permute(3, 2, 0, 1)
        res['dw'] = (got_w, ref_w, A_w, 0.0, None)
        if row['sink']:
            res['db (sink)'] = (sink, ref_b + s0.double(), A_b + s0.double().abs(), 0.0, None)
        else:
            res['db'] = (db, ref_b, A_b, 0.0, None)
        prim = dw
    else:       # spade: gamma | beta = conv(x, w, b) with 2C couts; mix = instnorm(z) (1 + gamma) + beta
        C = Co
        w = rnd((2 * C, Ci, k, k), 2 + seed, (Ci * k * k) ** -0.5); b = rnd((2 * C,), 3 + seed, 0.1)
        wt = tck(w)
        z = rnd((N, C, H, W), 6 + seed)
        img = wino_image(hip, wt, Ci, 2 * C, 0, spadeC=C) if row['img'] == 'wino' else None
        hip.launch_counts(reset=True)
        zd = z.to(DEV).contiguous(memory_format=torch.channels_last).to(xdt)
        xd = x.to(DEV).contiguous(memory_format=torch.channels_last).to(xdt)
        r = hip.gb_spade_fwd(xd, wt, b.to(DEV), zd, 1e-5, w_bf16=hip.cast_bf16(tkc(w)) if bf else None, w_wino=img)
        c = counted(hip)
        assert r is not None, 'the fused SPADE path declined'
        mix, gamma, mean, rstd = r
        gb, A = CC.fwd_ref(x_in(x), w_in(w), b, 1, 1)
        zr = x_in(z)
        m64 = zr.mean((2, 3)); s64 = (zr.var((2, 3), unbiased=False) + 1e-5).rsqrt()
        assert float(((mean.cpu().double().reshape(N, C) - m64).abs() / (zr.std((2, 3)) + 1e-30)).max()) <= 1e-5, 'instance mean'
        assert float(((rstd.cpu().double().reshape(N, C) - s64).abs() / s64).max()) <= 1e-5, 'instance rstd'
        zn = (zr - mean.cpu().double().reshape(N, C, 1, 1)) * rstd.cpu().double().reshape(N, C, 1, 1)      # (the statistics as the kernel read them)
        g_, be = gb[:, :C], gb[:, C:]
        ref_mix = zn * (1 + g_) + be
        zs = (zr.abs() + mean.cpu().double().reshape(N, C, 1, 1).abs()) * rstd.cpu().double().reshape(N, C, 1, 1)      # scale of z rstd - mean rstd in fp32
        A_mix = zs * (A[:, :C] + (1 + g_).abs()) + A[:, C:] + be.abs()
        # bf16: gamma | beta are rounded to bf16 before the modulation (as the two-step path stores them): u_out of each, like a stored result
        extra = CC.U_BF16 * (zs * g_.abs() + be.abs()) if bf else None
        res['gamma'] = (gamma, g_, A[:, :C], u_y, None)
        res['mix'] = (mix, ref_mix, A_mix, u_y, extra)
        prim = mix
    return res, c, prim


def kernels_in_fresh_process(rid):
    """the kernels (hip.dynamic_lds names) a new process launches for row `rid` alone (the table is per process and never reset)"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ('import sys, json\n'
            f'sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]\n'
            'import torch, mrdis, test_gpu_conv_paths as T\n'
            f'row = next(p.values[0] for p in T.ROWS if p.id == {rid!r})\n'
            'hip = mrdis.hip\n'
            'for k, v in row["opts"].items():\n    hip.set_option(k, v)\n'
            'T.run_row(hip, row)\ntorch.cuda.synchronize()\n'
            'print(json.dumps(sorted(hip.dynamic_lds())))\n')
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return set(json.loads(r.stdout.strip().splitlines()[-1]))


@pytest.mark.parametrize('row', ROWS)
def test_conv_path(mrdis, row, request):
    hip = mrdis.hip
    for name, v in row['opts'].items():
        hip.set_option(name, v)
    fell = hip.fallbacks['conv2d_bwd_weight_bf16']
    res, c, prim = run_row(hip, row)
    expect = set(row['expect'])
    fam = {f: n for f, n in c.items() if f != 'all'}
    assert all(fam[f] > 0 for f in expect) and all(n == 0 for f, n in fam.items() if f not in expect), (row['expect'], {f: n for f, n in fam.items() if n})
    assert hip.fallbacks['conv2d_bwd_weight_bf16'] - fell == (1 if row['fallback'] else 0), 'the bf16 weight-gradient fallback'
    if row['expect'] and row['expect'][0].startswith('bwgrad'):
        assert fam[row['expect'][0]] == 1, fam[row['expect'][0]]               # counted once per launch
    if row['launches'] is not None:
        assert c['all'] == row['launches'], (row['launches'], c['all'])
    kappa = KAPPA[(row['kname'], row['op'])]
    for name, (got, ref, A, u_out, extra) in res.items():
        r = CC.ratio(got, ref, A, u_out, extra)
        rec = dict(row=request.node.callspec.id, kernel=row['kname'], op=row['op'], out=name, ratio=r, kappa=kappa)
        if os.environ.get('MRDIS_DUMP_MEASURED') and row['kname'].startswith('bwgrad'):        # beside it, the plain fp32 evaluation kappa derives from
            rec['yardstick'] = wgrad_yardstick(row)['dw' if name == 'dw' else 'db']
        dump_measured('conv_path_margins.jsonl', rec)
        CC.check(got, ref, A, kappa, u_out, extra, what=f'{row["kname"]} {row["op"]} {name}')
    if row['lds_kernel'] is not None:
        names = kernels_in_fresh_process(request.node.callspec.id)
        assert row['lds_kernel'] in names and 'tapconv_kernel' not in names, names
    if row['chain'] is not None:
        for name, v in row['chain'].items():
            hip.set_option(name, v)
        _, c2, prim2 = run_row(hip, row)
        assert not torch.equal(prim.float(), prim2.float()), f'{row["kname"]}: the same bits as the kernel the options {row["chain"]} pick'
    if row['twin'] is not None:
        topts, tfam = row['twin']
        assert tfam not in expect
        for name, v in topts.items():
            hip.set_option(name, v)
        res2, c2, _ = run_row(hip, row)
        assert {f for f, n in c2.items() if n and f != 'all'} == {tfam}, (tfam, {f: n for f, n in c2.items() if n})
        for name in res:
            assert torch.equal(res[name][0], res2[name][0]), f'{name}: {row["kname"]} and {tfam} differ in some bit'


def test_table_covers_every_family(mrdis):
    """every counted family of hip.KERNEL_FAMILIES is the expected family of a row, or is listed in NOT_IN_TABLE with its reason"""
    fams = set(mrdis.hip.KERNEL_FAMILIES)
    in_table = {f for p in ROWS for f in p.values[0]['expect']}
    assert in_table | set(NOT_IN_TABLE) == fams and not (in_table & set(NOT_IN_TABLE)), (fams - in_table - set(NOT_IN_TABLE), in_table & set(NOT_IN_TABLE))
    for p in ROWS:
        row = p.values[0]
        assert (row['kname'], row['op']) in KAPPA, p.id
        # an uncounted row proves its kernel by a different result from the next kernel (chain), by its launch count, by having no fallback
        # (mixed storage), or by being the last kernel of the dispatcher's order
        assert (row['expect'] or row['chain'] or row['launches'] or row['lds_kernel'] or row['dtype'] in MIXED or row['kname'] in TERMINAL
                or p.id in SAME_BITS), p.id


# ---------------------------------------------------------------- the bf16 weight gradients through the C ABI (mrdis_conv2d_bwd_weight)
EUNSUPPORTED, EWORKSPACE, EALIGN = -2, -3, -5          # include/mrdis.h
GUARD = 64          # floats on each side of dw and dbias


def _abi_call(hip, geom, dw, db, ws=None, ws_bytes=None, accumulate=0, seed=0):
    """mrdis_conv2d_bwd_weight on bf16 channel slices of the row's operands -> the return code"""
    import bwgrad_plan as P
    lib = hip.load()
    N, Ci, Co, H, W, k, st, pad = geom
    Ho, Wo = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
    x, ldx = hip.nhwc(in_slice(rnd((N, Ci, H, W), 1 + seed), B16, 11))
    dy, lddy = hip.nhwc(in_slice(rnd((N, Co, Ho, Wo), 4 + seed), B16, 13))
    if ws is None:
        nb = max(int(lib.mrdis_conv2d_bwd_weight_workspace(N, H, W, Ci, Co, k, k, st, pad)), (P.plan(N, Ci, Co, H, W, k, st, pad) or {'ws': 0})['ws'], 16)
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    rc = lib.mrdis_conv2d_bwd_weight(x.data_ptr(), ldx, dy.data_ptr(), lddy, dw.data_ptr(), db.data_ptr(), ws.data_ptr(),
                                     ws.numel() if ws_bytes is None else ws_bytes, N, H, W, Ci, Co, k, k, st, pad, accumulate, hip.DT_BF16, hip._stream())
    torch.cuda.synchronize()
    return rc


def _guarded(n):
    """(a NaN-prefilled fp32 buffer of n + 2 GUARD floats, its n-float middle)"""
    buf = torch.full((n + 2 * GUARD,), float('nan'), device=DEV)
    return buf, buf[GUARD:GUARD + n]


def test_bwgrad_abi_refusals_launch_nothing(mrdis):
    """what the bf16 weight-gradient family refuses comes back as a code with no kernel launched ('all' unchanged): a workspace one byte short of
    what the planned slabs need, a workspace that is not 16-byte aligned, and bf16 views outside its domain -- Co = 12, Ci = 48, 4x4 maps whose
    eight-image tile has too many halo positions, stride 2 on an odd height (bf16 views have no fp32 kernel behind them in the C call: the
    Python wrapper owns that fallback)"""
    import bwgrad_plan as P
    hip = mrdis.hip
    lib = hip.load()

    def refused(geom, want, **kw):
        N, Ci, Co = geom[:3]
        k = geom[5]
        dw, db = torch.zeros(k * k * Ci * Co, device=DEV), torch.zeros(Co, device=DEV)
        hip.launch_counts(reset=True)
        rc = _abi_call(hip, geom, dw, db, **kw)
        c = hip.launch_counts()
        assert rc == want and c['all'] == 0, (geom, rc, want, c['all'])
        assert not dw.any() and not db.any()

    geom = (8, 16, 40, 34, 38, 4, 2, 1)                                         # 'bwgrad_s2<1,2,HALF> 4x4': 40 slabs
    need = P.plan(*geom[:5], k=4, stride=2)['ws']
    # for this layer the slabs of this family are the largest request of any weight-gradient kernel, so the library's figure is this family's
    # and one byte less is refused by run_bwgrad_s2 itself
    assert need == 4 * 40 * (16 * 16 * 40 + 40) + 256 == int(lib.mrdis_conv2d_bwd_weight_workspace(8, 34, 38, 16, 40, 4, 4, 2, 1))
    ws = torch.empty(need + 32, dtype=torch.uint8, device=DEV)
    refused(geom, EWORKSPACE, ws=ws, ws_bytes=need - 1)
    refused(geom, EALIGN, ws=ws[8:], ws_bytes=need)
    refused((2, 96, 72, 129, 33, 3, 1, 1), EWORKSPACE, ws_bytes=P.plan(2, 96, 72, 129, 33)['ws'] - 1)      # stride 1, 43 slabs (the buffer itself is full size)
    refused((2, 96, 12, 129, 33, 3, 1, 1), EUNSUPPORTED)                        # Co % 8 != 0
    refused((2, 48, 72, 129, 33, 3, 1, 1), EUNSUPPORTED)                        # Ci % 32 != 0 and not 16
    refused((256, 32, 64, 4, 4, 3, 1, 1), EUNSUPPORTED)                         # 4096 positions, but 8 x 6 x 6 halo positions per tile
    refused((8, 32, 24, 33, 38, 3, 2, 1), EUNSUPPORTED)                         # stride 2, odd H
    dw, db = torch.zeros(16 * 16 * 40, device=DEV), torch.zeros(40, device=DEV)   # and with exactly the bytes it needs the same call runs
    hip.launch_counts(reset=True)
    assert _abi_call(hip, geom, dw, db, ws=ws, ws_bytes=need) == 0
    c = hip.launch_counts()
    assert c['bwgrad_s2'] == 1 and c['all'] == 2 and dw.any() and db.any()


@pytest.mark.parametrize('geom,fam', [((1, 16, 40, 65, 65, 3, 1, 1), 'bwgrad'), ((2, 96, 72, 129, 33, 3, 1, 1), 'bwgrad3'), ((8, 16, 40, 34, 38, 4, 2, 1), 'bwgrad_s2')],
                         ids=['bwgrad<1,2,__bf16,HALF>', 'bwgrad3<1,2> cout tail 72', 'bwgrad_s2<1,2,HALF>'])
def test_bwgrad_abi_stores_stay_inside_dw_and_dbias(mrdis, geom, fam):
    """dw and dbias in the middle of NaN-prefilled buffers: the 64 floats on each side keep their bits (a HALF block's rows 16 .. 31 and the
    couts 72 .. 127 of a cout tail have nowhere to go), the middles equal what the wrapper returns for the same call (checked against float64 by
    the row of this geometry), and accumulate_bias adds exactly: prefill + db"""
    hip = mrdis.hip
    N, Ci, Co, H, W, k, st, pad = geom
    wbuf, dw = _guarded(k * k * Ci * Co)
    bbuf, db = _guarded(Co)
    hip.launch_counts(reset=True)
    assert _abi_call(hip, geom, dw, db) == 0
    c = hip.launch_counts()
    assert c[fam] == 1 and c['all'] == 2, {f: n for f, n in c.items() if n}
    nan = torch.full((1,), float('nan')).view(torch.int32).item()
    for buf in (wbuf, bbuf):
        sides = torch.cat([buf[:GUARD], buf[-GUARD:]]).view(torch.int32)
        assert bool((sides == nan).all()), 'a store landed outside dw / dbias'
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()
    Ho, Wo = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
    dw_w, db_w = hip.conv2d_bwd_weight(in_slice(rnd((N, Ci, H, W), 1), B16, 11), in_slice(rnd((N, Co, Ho, Wo), 4), B16, 13), k, k, st, pad, need_bias=True)
    assert torch.equal(dw_w.reshape(-1), dw) and torch.equal(db_w, db)
    pre = rnd((Co,), 7).to(DEV)
    acc = pre.clone()
    wbuf2, dw2 = _guarded(k * k * Ci * Co)
    assert _abi_call(hip, geom, dw2, acc, accumulate=1) == 0
    assert torch.equal(acc, pre + db) and torch.equal(dw2, dw)
