"""Element-wise float64 check of a convolution result (no GPU needed).

For a result `got` of an operation whose exact value is `ref` (float64, computed from the operands the kernel actually multiplies: bf16-rounded
where the kernel reads bf16), every element must satisfy

    |got - ref| <= kappa * u * A  +  u_out * |ref|  +  extra  +  tiny

  * A      the same operation in float64 on absolute values (conv(|x|, |w|) + |b| for the forward, likewise for the data gradient, sum |x| |dy|
           for the weight gradient, sum |dy| for the bias): the standard per-element scale of a dot product's rounding error;
  * u      2^-24, fp32 accumulation;
  * u_out  2^-8 for a bf16 output (the rounding of the stored result), 0 for fp32;
  * extra  what a caller knows its path rounds on top (e.g. bf16 gamma | beta before the SPADE modulation), default 0.

LeakyReLU applies to ref only; A stays as it is (the slope is <= 1).  Unlike a bound scaled by the largest output (tests/test_gpu_ops.py close()),
this one catches a fault confined to a few channels or rows at a level well above rounding (tests/test_conv_check.py plants such faults)."""
import torch
import torch.nn.functional as F

U = 2.0 ** -24          # fp32 accumulation
U_BF16 = 2.0 ** -8      # a result stored as bf16
TINY = 1e-30
SLOPE = 0.2


def bf16_round(t):
    """the value a bf16 view of t holds (round to nearest even), as float64"""
    return t.detach().to(torch.bfloat16).double()


def fwd_ref(x, w, b, stride, pad, lrelu=False):
    """x (N, Ci, H, W), w (Co, Ci, kh, kw), b (Co,) or None, all float64 -> (ref, A)"""
    x, w = x.double(), w.double()
    ref = F.conv2d(x, w, None if b is None else b.double(), stride, pad)
    A = F.conv2d(x.abs(), w.abs(), None if b is None else b.double().abs(), stride, pad)
    if lrelu:
        ref = F.leaky_relu(ref, SLOPE)
    return ref, A


def dgrad_ref(dy, w, in_hw, stride, pad):
    """data gradient of conv2d(x, w, stride, pad) for x of spatial extent in_hw -> (ref, A)"""
    dy, w = dy.double(), w.double()
    shape = (dy.shape[0], w.shape[1]) + tuple(in_hw)
    ref = torch.nn.grad.conv2d_input(shape, w, dy, stride, pad)
    A = torch.nn.grad.conv2d_input(shape, w.abs(), dy.abs(), stride, pad)
    return ref, A


def wgrad_ref(x, dy, kh, kw, stride, pad):
    """(dw (Co, Ci, kh, kw), A_dw, db (Co,), A_db)"""
    x, dy = x.double(), dy.double()
    shape = (dy.shape[1], x.shape[1], kh, kw)
    dw = torch.nn.grad.conv2d_weight(x, shape, dy, stride, pad)
    A = torch.nn.grad.conv2d_weight(x.abs(), shape, dy.abs(), stride, pad)
    return dw, A, dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3))


def wgrad_fp32(x, dy, k, stride, pad, rounded_bias=True):
    """the weight and bias gradient of a bf16 kernel's operands in plain fp32 on the CPU -> (dw (Co, Ci, k, k), db (Co,)), both fp32: torch's own
    convolution on the bf16-rounded x and dy (their products are exact in fp32, so only the order of the fp32 sums differs from a kernel's), the
    bias summed from the rounded dy (bf16 views) or from dy as it is (rounded_bias=False: fp32 views whose kernel rounds after summing)"""
    xb, yb = x.to(torch.bfloat16).float(), dy.to(torch.bfloat16).float()
    dw = torch.nn.grad.conv2d_weight(xb, (dy.shape[1], x.shape[1], k, k), yb, stride, pad)
    return dw, (yb if rounded_bias else dy.float()).sum((0, 2, 3))


def fwd_ref3d(x, w, b, stride, pad, residual=None):
    """x (N, Ci, D, H, W), w (Co, Ci, kd, kh, kw), b (Co,) or None, residual (N, Co, Do, Ho, Wo) or None -> (ref, A); a fused residual adds |res| to A"""
    x, w = x.double(), w.double()
    ref = F.conv3d(x, w, None if b is None else b.double(), stride, pad)
    A = F.conv3d(x.abs(), w.abs(), None if b is None else b.double().abs(), stride, pad)
    if residual is not None:
        ref = ref + residual.double()
        A = A + residual.double().abs()
    return ref, A


def dgrad_ref3d(dy, w, in_dhw, stride, pad):
    """data gradient of conv3d(x, w, stride, pad) for x of spatial extent in_dhw -> (ref, A)"""
    dy, w = dy.double(), w.double()
    shape = (dy.shape[0], w.shape[1]) + tuple(in_dhw)
    ref = torch.nn.grad.conv3d_input(shape, w, dy, stride, pad)
    A = torch.nn.grad.conv3d_input(shape, w.abs(), dy.abs(), stride, pad)
    return ref, A


def wgrad_ref3d(x, dy, k, stride, pad):
    """(dw (Co, Ci, k, k, k), A_dw, db (Co,), A_db)"""
    x, dy = x.double(), dy.double()
    shape = (dy.shape[1], x.shape[1], k, k, k)
    dw = torch.nn.grad.conv3d_weight(x, shape, dy, stride, pad)
    A = torch.nn.grad.conv3d_weight(x.abs(), shape, dy.abs(), stride, pad)
    return dw, A, dy.sum((0, 2, 3, 4)), dy.abs().sum((0, 2, 3, 4))


def ratio(got, ref, A, u_out=0.0, extra=None):
    """worst (|got - ref| - u_out |ref| - extra) / (u A) over the elements: the kappa this result needs (inf for a non-finite element)"""
    got = got.detach().double().cpu()
    ref, A = ref.double().cpu(), A.double().cpu()
    assert got.shape == ref.shape == A.shape, (got.shape, ref.shape, A.shape)
    if not torch.isfinite(got).all():
        return float('inf')
    excess = (got - ref).abs() - u_out * ref.abs() - TINY
    if extra is not None:
        excess = excess - extra.double().cpu()
    return max(float((excess / (U * A + TINY)).max()), 0.0)


def check(got, ref, A, kappa, u_out=0.0, extra=None, what=''):
    """assert the element-wise bound; returns the measured ratio (the kappa the result needed)"""
    got_d = got.detach().double().cpu()
    ref, A = ref.double().cpu(), A.double().cpu()
    assert got_d.shape == ref.shape, (what, got_d.shape, ref.shape)
    bound = kappa * U * A + u_out * ref.abs() + TINY
    if extra is not None:
        bound = bound + extra.double().cpu()
    bad = ~((got_d - ref).abs() <= bound)            # (NaN fails)
    if bad.any():
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements outside kappa = {kappa} (first at {idx}: got {float(got_d[idx])!r}, '
                             f'ref {float(ref[idx])!r}, bound {float(bound[idx]):.3e}); worst ratio {ratio(got_d, ref, A, u_out, extra):.1f}')
    return ratio(got_d, ref, A, u_out, extra)


# kappa per (kernel family or uncounted path, direction) of the rows of tests/test_gpu_conv_paths.py: about 4x the worst measured ratio (in the comment; profiles/conv_path_margins.txt), at least 1.
# The F(4x4) forms (wino4*, 16 - 43) amplify rounding through their transforms about 10x more than F(2x2) and the direct kernels (1 - 6): their
# kappa is large and, in fp32, the element-wise bound adds little over close() for them -- there the row's value is the proof of which kernel ran.
# The bf16 rows measure below 1 once the output rounding (u_out |ref|) is taken off: there the bound is essentially that rounding.
# c4_mixed (24 - 35, against 4 for the fp32-output c4 kernel) is by design: the bf16-output form of c4conv carries both fp32 operands as TWO bf16
# terms and sums three products (2^-16 relative per product, csrc/mrdis_conv.hip c4conv_body OBF16), still far under the 2^-8 of its bf16 output.
KAPPA = {
    ('wino', 'fwd'):                10,    #   2.36
    ('wino', 'dgrad'):               7,    #   1.73
    ('wino2', 'fwd'):               15,    #   2.94
    ('wino2', 'dgrad'):              8,    #   1.97
    ('wino4', 'fwd'):              200,    #  42.65
    ('wino4', 'dgrad'):            150,    #  33.06
    ('wino4n', 'fwd'):              90,    #  21.88
    ('wino4r', 'fwd'):             200,    #  42.64
    ('wino2_spade', 'spade'):        8,    #   1.80
    ('wino4_spade', 'spade'):      200,    #  41.18
    ('wino_wgrad', 'wgrad'):         3,    #   0.74
    ('wino_wgrad2', 'wgrad'):        9,    #   2.20
    ('wino4_wgrad', 'wgrad'):       65,    #  15.85
    ('bconv3', 'fwd'):               1,    #   0.02
    ('bconv3', 'dgrad'):             2,    #   0.33
    ('bconv4', 'fwd'):               1,    #   0.05
    ('bconv4', 'dgrad'):             2,    #   0.33
    ('bconv3_spade', 'spade'):       1,    #   0.12
    ('bconv4_spade', 'spade'):       1,    #   0.14
    ('split6_c4', 'fwd'):           15,    #   3.33
    ('split6_co4', 'fwd'):           4,    #   0.94
    ('split6_co4', 'dgrad'):         3,    #   0.75
    ('split6_c16', 'fwd'):          20,    #   4.28
    ('split6_wgrad16', 'wgrad'):     1,    #   0.09
    ('split6_tap', 'fwd'):          20,    #   4.26
    ('split6_tap', 'dgrad'):        20,    #   4.66
    ('direct', 'fwd'):              20,    #   3.78
    ('direct', 'dgrad'):            15,    #   2.99
    ('direct_s2', 'dgrad'):         15,    #   3.69
    ('c4', 'fwd'):                  15,    #   3.72
    ('co4', 'fwd'):                  5,    #   1.20
    ('co4', 'dgrad'):                5,    #   1.21
    ('c16', 'fwd'):                 25,    #   5.75
    ('pw', 'fwd'):                  10,    #   2.45
    ('pw', 'dgrad'):                15,    #   3.24
    ('pw', 'wgrad'):                 1,    #   0.11
    ('s2', 'fwd'):                  20,    #   4.70
    ('s2', 'dgrad'):                15,    #   3.74
    ('wgrad', 'wgrad'):              6,    #   1.44
    ('wgrad16', 'wgrad'):            1,    #   0.06
    ('wgrad_c4', 'wgrad'):           1,    #   0.08
    ('wgrad_s2', 'wgrad'):           1,    #   0.12
    ('bconv', 'fwd'):                1,    #   0.00
    # the bf16 weight-gradient family (csrc/mrdis_bf16.hip): 4x the worst ratio of the rows' sums in plain fp32 on the CPU (wgrad_fp32; the
    # yardstick in the comment), NOT of the kernels -- tests/test_conv_check.py holds these four to the yardstick where it runs; the kernels'
    # own ratios stand beside it in profiles/conv_path_margins.txt.  (The 0.24 once recorded for 'bwgrad' was the fp32 generic kernel's: its
    # only row fell back to it, and is now the 'wgrad' row 'wgrad bf16 tiny-map fallback'.)
    ('bwgrad', 'wgrad'):            10,    #   2.43  bwgrad<2,1,float>
    ('bwgrad2', 'wgrad'):           18,    #   4.29  <2,2> many-image tiles
    ('bwgrad3', 'wgrad'):           18,    #   4.29  <2,2> many-image tiles
    ('bwgrad_s2', 'wgrad'):          4,    #   0.99  bwgrad_s2<1,1,false> 3x3
    ('wgrad16_bf16', 'wgrad'):       1,    #   0.05
    ('pw_mixed', 'fwd'):            10,    #   2.31
    ('pw_mixed', 'dgrad'):           1,    #   0.00
    ('pw_mixed', 'wgrad'):           1,    #   0.14
    ('co4_mixed', 'fwd'):            4,    #   0.82
    ('co4_mixed', 'dgrad'):          4,    #   0.78
    ('c4_mixed', 'fwd'):           100,    #  24.47
    ('c4_mixed', 'dgrad'):         150,    #  35.43
    ('wgrad_co4b', 'wgrad'):         1,    #   0.07
    ('wgrad_c4_mixed', 'wgrad'):     1,    #   0.07
    # 3-D (tests/test_gpu_conv3d_paths.py; profiles/conv3d_path_margins.txt).  'wino_spade' is the hybrid 3-D Winograd (F(2x2) in (h, w), direct
    # in depth) under the name its counter carries; 'direct3d_s2' the tap-table kernel on the eight stride-2 parity classes of the data gradient.
    ('split6_c3d', 'fwd'):          20,    #   4.09
    ('split6_c3d', 'dgrad'):        25,    #   5.21
    ('split6_w3d', 'wgrad'):         1,    #   0.10
    ('c3d16', 'fwd'):               25,    #   5.62
    ('c3d16', 'dgrad'):             20,    #   4.26
    ('direct3d', 'fwd'):            25,    #   5.62
    ('direct3d', 'dgrad'):          15,    #   3.37
    ('direct3d_s2', 'dgrad'):       15,    #   3.63
    ('wino_spade', 'fwd'):           8,    #   1.86
    ('wino_spade', 'dgrad'):         6,    #   1.36
    ('wino_wgrad3d', 'wgrad'):      25,    #   5.87
    ('wgrad3d', 'wgrad'):            7,    #   1.75
    ('wgrad3d16', 'wgrad'):          5,    #   1.15
}
