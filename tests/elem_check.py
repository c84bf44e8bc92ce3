"""Float64 references and error scales of the statistics, norm and resize kernels (csrc/mrdis_elem.hip); no GPU needed.

The bound is the one of tests/conv_check.py (check / ratio / U / U_BF16 / bf16_round are its own, imported, not copied):

    |got - ref| <= kappa * u * A  +  u_out * |ref|  +  extra  +  tiny

Every function returns (ref, A) in float64: ref from the operands the kernel actually reads (bf16-rounded by the caller where storage is
bf16), A the same expression on the absolute value of every term.  Tensors are logical (N, C, H, W); statistics are (G * C,), group-major,
as the kernels store them.  Per operation:

  * column statistics over the P rows of a (group, channel): mean has A = mean|x|.  The kernel returns rstd = 1 / sqrt(var + eps); the variance
    is recovered as 1 / rstd^2 - eps and checked against the float64 variance with A_var = mean(x^2) + mean^2 -- the honest scale of a
    ONE-PASS variance E[x^2] - mean^2 (a mean 30 sigma from zero makes A_var 1800 x the variance: that loss is the algorithm's, and the bound
    says so) -- plus `rstd_rounding`, what one fp32 rounding of rstd does to the recovered variance: 2 u (var + eps).
  * running statistics (nn.BatchNorm2d): (1 - momentum) running + momentum stat, the variance unbiased (P / (P - 1); P == 1 left biased);
    in the grouped form the running value is rounded to fp32 between the groups, as G separate calls round it.  A follows term by term.  The
    grouped form is in addition held to the bits of G separate calls (assert_same_bits): a missing rounding between groups is a half-ulp
    matter that no bound with kappa >= 1 can see.
  * apply steps (BatchNorm train / eval, SPADE forward): (x - m) rstd gamma + beta, (z - m) rstd (1 + g) + b, with
    A = (|x| + |m|) rstd |gamma| + |beta|.  Checked twice: against the mean / rstd THE KERNEL RETURNED (a fault is then the apply kernel's),
    and end to end against float64 statistics with the statistics' own bound propagated (stats_propagated: d y / d m and d y / d rstd times
    what the statistics' kappas allow).
  * backward sums (sum dy, sum dy xhat; sum dzh, sum dzh zhat with dzh = dout (1 + g)): A = the sum of the absolute terms.
    dx = gamma rstd (dy - s0 / P - xhat s1 / P) and dz likewise are formed term by term from float64 sums; what the sums' own bound allows
    comes back as `extra` (sums_propagated).  d gamma = dout zhat per element for SPADE; d beta = dout is a copy (bits).
    acc_dgamma / acc_dbeta: the sink's value plus the groups' sums in order.
  * SPADE backward through the x2 resize: d x = U^T d z, U^T the adjoint of F.interpolate (float64 autograd; its weights are >= 0, so A is U^T of
    d z's A).  z is U x -- in the bf16 form the bf16-rounded U x, as up2_value stores it.  The one-pass route forms U^T z as (U^T U) x from the
    unrounded low-resolution map: in bf16 that differs from U^T of the rounded z by up to 2^-8 U^T|z| (s1 / HW) rstd^2, returned as `extra`.
    With exact statistics the expression equals autograd through interpolate -> instance_norm -> modulation (tests/test_elem_check.py).
  * bilinear forward / backward: float64 F.interpolate and its autograd; A the same on |x| / |dy|.  The kernels form the source index in fp32
    as ATen does, so each weight is off by up to delta = 4 u (src + 1) (four fp32 roundings on the way to the index).  Against A alone that
    measured up to 1.6e6 -- in the kernels and in fp32 torch alike: where an input pixel's weight is itself ~1e-4, delta is as large as the
    weight -- so a general resize carries `extra` = delta times the lines the moved index can draw on (bilinear_index_extra / _bwd_index_extra);
    the exact x2 geometry and the identity have exact weights and take none.
  * x2 resize with instance statistics: y as the bilinear forward; the statistics as column statistics of the y that was STORED."""
import torch
import torch.nn.functional as F

from conv_check import U, U_BF16, TINY, bf16_round, check, ratio      # noqa: F401  (re-exported: one bound for both tables)


# ---------------------------------------------------------------- column statistics
def _grouped(x, groups):
    N, C, H, W = x.shape
    assert N % groups == 0
    return x.double().reshape(groups, N // groups, C, H, W)


def stats_ref(x, groups, eps):
    """x (N, C, H, W), `groups` equal sample blocks -> {mean: (ref, A), var: (ref, A), rstd: ref, P}; all (groups * C,)"""
    g = _grouped(x, groups)
    P = g.shape[1] * g.shape[3] * g.shape[4]
    m = g.mean((1, 3, 4))
    ex2 = (g * g).mean((1, 3, 4))
    var = ((g - m[:, None, :, None, None]) ** 2).mean((1, 3, 4))          # two-pass in float64: exact to ~1e-16 whatever the mean
    return dict(mean=(m.reshape(-1), g.abs().mean((1, 3, 4)).reshape(-1)), var=(var.reshape(-1), (ex2 + m * m).reshape(-1)),
                rstd=(var + eps).rsqrt().reshape(-1), P=P)


def var_from_rstd(rstd, eps):
    return 1.0 / rstd.detach().double().cpu() ** 2 - eps


def rstd_rounding(var_ref, eps):
    """what one fp32 rounding of rstd does to 1 / rstd^2"""
    return 2.0 * U * (var_ref + eps)


def running_ref(run_mean0, run_var0, mean, var, A_mean, A_var, P, momentum, groups):
    """nn.BatchNorm2d called once per group, in order: -> (run_mean, A, run_var, A), each (C,)"""
    C = run_mean0.numel()
    rm, rv = run_mean0.double(), run_var0.double()
    Am, Av = rm.abs(), rv.abs()
    unb = P / (P - 1.0) if P > 1 else 1.0
    mean, var, A_mean, A_var = (t.reshape(groups, C) for t in (mean, var, A_mean, A_var))
    for g in range(groups):
        rm = ((1 - momentum) * rm + momentum * mean[g]).float().double()
        rv = ((1 - momentum) * rv + momentum * unb * var[g]).float().double()
        Am = (1 - momentum) * Am + momentum * A_mean[g] + (rm.abs() if g < groups - 1 else 0)          # the rounding between groups
        Av = (1 - momentum) * Av + momentum * unb * A_var[g] + (rv.abs() if g < groups - 1 else 0)
    return rm, Am, rv, Av


def assert_same_bits(got, want, what):
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    it = torch.int32 if got.dtype is torch.float32 else torch.int16
    bad = got.view(it) != want.view(it)
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} of {bad.numel()} elements differ in their bits'


# ---------------------------------------------------------------- apply steps
def _per_row(stat, x, groups):
    """(groups * C,) -> broadcastable over x (N, C, H, W), sample n using group n // (N / groups)"""
    N, C = x.shape[:2]
    return stat.detach().double().cpu().reshape(groups, 1, C).expand(groups, N // groups, C).reshape(N, C, 1, 1)


def norm_apply_ref(x, mean, rstd, groups, gamma=None, beta=None):
    """BatchNorm: (x - mean) rstd gamma + beta, gamma / beta (C,) or None; the statistics as given"""
    x = x.double()
    m, r = _per_row(mean, x, groups), _per_row(rstd, x, groups)
    g = 1.0 if gamma is None else gamma.double().reshape(1, -1, 1, 1)
    b = 0.0 if beta is None else beta.double().reshape(1, -1, 1, 1)
    return (x - m) * r * g + b, (x.abs() + m.abs()) * r * abs(g) + abs(b) + 0 * x


def bn_eval_ref(x, run_mean, run_var, eps, gamma=None, beta=None):
    return norm_apply_ref(x, run_mean.double(), (run_var.double() + eps).rsqrt(), 1, gamma, beta)


def spade_fwd_ref(z, g, b, mean, rstd):
    """(z - mean) rstd (1 + g) + b; g, b maps like z; statistics (N * C,)"""
    z, g, b = z.double(), g.double(), b.double()
    m, r = _per_row(mean, z, z.shape[0]), _per_row(rstd, z, z.shape[0])
    return (z - m) * r * (1 + g) + b, (z.abs() + m.abs()) * r * (1 + g.abs()) + b.abs()


def stats_propagated(x, st, groups, scale, k_mean, k_var, eps):
    """the `extra` of an end-to-end check of y = (x - m) rstd scale: |dy/dm| dm + |dy/drstd| drstd for statistics inside their own bound
    (dm <= k_mean u A_mean; dvar <= k_var u A_var + rstd_rounding; drstd = rstd^3 dvar / 2).  scale: |gamma| (C,) or None, or a map |1 + g|"""
    x = x.double()
    m, r = _per_row(st['mean'][0], x, groups), _per_row(st['rstd'], x, groups)
    dm = k_mean * U * _per_row(st['mean'][1], x, groups)
    dvar = k_var * U * _per_row(st['var'][1], x, groups) + _per_row(rstd_rounding(st['var'][0], eps), x, groups)
    s = 1.0 if scale is None else (scale.double().abs().reshape(1, -1, 1, 1) if scale.dim() == 1 else scale.double().abs())
    return (r * dm + (x - m).abs() * 0.5 * r ** 3 * dvar) * s + 0 * x


# ---------------------------------------------------------------- backward
def bwd_sums_ref(d, x, mean, rstd, groups, g=None):
    """per (group, channel): s0 = sum dh, s1 = sum dh xhat, dh = d (1 + g) (g None: dh = d), xhat = (x - mean) rstd -> (s0, A0, s1, A1), (groups * C,)"""
    d, x = d.double(), x.double()
    m, r = _per_row(mean, x, groups), _per_row(rstd, x, groups)
    dh, dha = (d, d.abs()) if g is None else (d * (1 + g.double()), d.abs() * (1 + g.double().abs()))
    red = lambda t: _grouped(t, groups).sum((1, 3, 4)).reshape(-1)
    return red(dh), red(dha), red(dh * (x - m) * r), red(dha * (x.abs() + m.abs()) * r)


def bwd_apply_ref(d, x, mean, rstd, groups, s0, s1, P, gamma=None, g=None):
    """scale rstd (dh - s0 / P - xhat s1 / P): scale = gamma (C,) (BatchNorm) or 1 (SPADE, where dh = d (1 + g)); sums as given -> (ref, A)"""
    d, x = d.double(), x.double()
    m, r = _per_row(mean, x, groups), _per_row(rstd, x, groups)
    a0, a1 = _per_row(s0, x, groups) / P, _per_row(s1, x, groups) / P
    sc = 1.0 if gamma is None else gamma.double().reshape(1, -1, 1, 1)
    dh, dha = (d, d.abs()) if g is None else (d * (1 + g.double()), d.abs() * (1 + g.double().abs()))
    xh, xha = (x - m) * r, (x.abs() + m.abs()) * r
    return sc * r * (dh - a0 - xh * a1), abs(sc) * r * (dha + a0.abs() + xha * a1.abs())


def sums_propagated(x, mean, rstd, groups, A0, A1, P, k_sum, gamma=None):
    """the `extra` of dx / dz formed from float64 sums: what sums inside their own bound (k_sum u A) move the result by"""
    x = x.double()
    m, r = _per_row(mean, x, groups), _per_row(rstd, x, groups)
    sc = 1.0 if gamma is None else gamma.double().abs().reshape(1, -1, 1, 1)
    return sc * r * k_sum * U * (_per_row(A0, x, groups) + ((x - m) * r).abs() * _per_row(A1, x, groups)) / P


def spade_dgamma_ref(d, z, mean, rstd):
    d, z = d.double(), z.double()
    m, r = _per_row(mean, z, z.shape[0]), _per_row(rstd, z, z.shape[0])
    return d * (z - m) * r, d.abs() * (z.abs() + m.abs()) * r


def acc_ref(acc0, sums, A, groups):
    """a sink that held acc0 (C,) after the G groups' sums (G * C,) were added in order"""
    C = acc0.numel()
    return acc0.double() + sums.double().reshape(groups, C).sum(0), acc0.double().abs() + A.double().reshape(groups, C).sum(0)


# ---------------------------------------------------------------- bilinear
def bilinear_ref(x, out_hw, align):
    x = x.double()
    f = lambda t: F.interpolate(t, size=tuple(out_hw), mode='bilinear', align_corners=bool(align))
    return f(x), f(x.abs())


def bilinear_bwd_ref(dy, in_hw, align):
    dy = dy.double()
    N, C = dy.shape[:2]
    x = torch.zeros((N, C) + tuple(in_hw), dtype=torch.float64, requires_grad=True)
    y = F.interpolate(x, size=tuple(dy.shape[2:]), mode='bilinear', align_corners=bool(align))
    dx, = torch.autograd.grad(y, x, dy, retain_graph=True)
    A, = torch.autograd.grad(y, x, dy.abs())
    return dx, A


def _axis(isz, osz, align):
    """ATen's source-index rule along one axis, in float64: (i0 per output index, the bound delta on what forming the index in fp32 moves it by).
    scale (a rounded quotient), scale * (o + 0.5), - 0.5 and 1 - l1 are one fp32 rounding each: |d src| <= 4 u (src + 1)"""
    o = torch.arange(osz, dtype=torch.float64)
    if align:
        src = ((isz - 1) / (osz - 1) if osz > 1 else 0.0) * o
    else:
        src = (isz / osz * (o + 0.5) - 0.5).clamp_min(0)
    return src.floor().long().clamp_max(isz - 1), 4 * U * (src + 1)


def _touched(t, dim, i0, delta, isz, adjoint=False):
    """delta(o) times the sum of the input lines i0 - 1 .. i0 + 2 (clamped) an output line can draw on once its index moves by delta -- one more on
    each side than the exact index reads: at an integer source index fp32 may step to the neighbouring pair; adjoint: the transposed map"""
    shape = [1] * t.dim(); shape[dim] = -1
    d = delta.reshape(shape)
    out = None
    if adjoint:
        size = list(t.shape); size[dim] = isz
        out = torch.zeros(size, dtype=torch.float64)
    for k in (-1, 0, 1, 2):
        idx = (i0 + k).clamp(0, isz - 1)
        if adjoint:
            out.index_add_(dim, idx, t * d)
        else:
            out = t.index_select(dim, idx) * d + (0 if out is None else out)
    return out


def bilinear_index_extra(x, out_hw, align):
    """the `extra` of a general resize: the kernels (like ATen in fp32) form the source index in fp32, so each weight is off by up to delta; the
    exact x2 geometry (weights 0.25 / 0.75) and the identity need none"""
    a = x.double().abs()
    Hi, Wi = a.shape[2:]
    Ho, Wo = out_hw
    (ih, dh), (iw, dw) = _axis(Hi, Ho, align), _axis(Wi, Wo, align)
    return _touched(bilinear_ref(a, (Hi, Wo), align)[0], 2, ih, dh, Hi) + _touched(bilinear_ref(a, (Ho, Wi), align)[0], 3, iw, dw, Wi)


def bilinear_bwd_index_extra(dy, in_hw, align):
    a = dy.double().abs()
    Ho, Wo = a.shape[2:]
    Hi, Wi = in_hw
    (ih, dh), (iw, dw) = _axis(Hi, Ho, align), _axis(Wi, Wo, align)
    return _touched(bilinear_bwd_ref(a, (Ho, Wi), align)[0], 2, ih, dh, Hi, True) + _touched(bilinear_bwd_ref(a, (Hi, Wo), align)[0], 3, iw, dw, Wi, True)


def up2(x, bf16=False):
    """z = U x, the x2 resize (align_corners = False) -- as stored: bf16-rounded in the bf16 form"""
    z = F.interpolate(x.double(), scale_factor=2, mode='bilinear', align_corners=False)
    return bf16_round(z) if bf16 else z


def spade_bwd_up2_ref(d, x, g, mean, rstd, k_sum, bf16=False, z=None, onepass=True):
    """SPADE backward with the x2 resize's adjoint inside: -> {dx: (ref, A, extra), dgamma: (ref, A)}; x the low-resolution map, d / g at
    full resolution, the statistics (of z = U x) as given; z: the stored U x where the caller holds it (else formed here).  extra: the sums' own bound, and in bf16 the one-pass route's unrounded U^T z"""
    z = up2(x, bf16) if z is None else z.double()
    N = z.shape[0]
    HW = z.shape[2] * z.shape[3]
    s0, A0, s1, A1 = bwd_sums_ref(d, z, mean, rstd, N, g)
    dz, A_dz = bwd_apply_ref(d, z, mean, rstd, N, s0, s1, HW, g=g)
    ex = sums_propagated(z, mean, rstd, N, A0, A1, HW, k_sum)
    if bf16 and onepass:          # (the two-pass routes read or re-form the rounded z: no such term)
        r = _per_row(rstd, z, N)
        ex = ex + U_BF16 * z.abs() * r * r * _per_row(s1, z, N).abs() / HW
    hw = tuple(x.shape[2:])
    dx, A = bilinear_bwd_ref(dz, hw, False)[0], bilinear_bwd_ref(A_dz, hw, False)[0]
    extra = bilinear_bwd_ref(ex, hw, False)[0]
    return dict(dx=(dx, A, extra), dgamma=spade_dgamma_ref(d, z, mean, rstd))


# kappa per (kernel or route, output) of the rows of tests/test_gpu_elem_paths.py: about 4x the worst measured ratio (in the comment, with the
# ratio of a plain fp32 torch evaluation on the CPU against the same float64 reference -- the yardstick -- after it; profiles/elem_path_margins.txt),
# at least 1.  Above 16x its yardstick measure only the variances (5.48 | 1.60 | 0.41 against 0.00): the kernels form E[x^2] - mean^2 from one pass, torch's
# var makes two -- the algorithm's property that A_var = mean(x^2) + mean^2 is there to absorb, and does on the mean-30-sigma rows (A_var = 1800 var; they
# measure 0.45 | 0.00).  A measured 0.00 means the row's `extra` (the statistics' or sums' own bound propagated, the fp32 source index of a general
# resize, the bf16 roundings) already covers the error: there the bound is essentially that term, and profiles/elem_path_margins.txt records beside it
# how much of `extra` the worst element uses (0.08 - 0.70; the two tight resize kernels 0.44 and 0.19).  The yardstick of the bf16 x2-adjoint rows
# (4202 | 4624) keeps z unrounded and so is not inside the bf16 model; it says nothing about the kernel, which reads the rounded z.
# SPADE d gamma through the x2 routes (8.03 against 2.86 for the plain kernel, yardstick 2.55) is d * zhat with zhat formed from an interpolated z:
# its A does not count the interpolation's own roundings, which the fp32 yardstick (reading the stored z) does not make.
KAPPA = {
    #                                  kappa     measured  yardstick
    ('stat_scalar', 'mean'):               5,    #   1.04      1.08
    ('stat_scalar', 'var'):                7,    #   1.28      0.00
    ('stat_scalar', 'run_mean'):           7,    #   1.72      1.76
    ('stat_scalar', 'run_var'):            8,    #   1.80      1.93
    ('bn', 'y apply'):                    15,    #   2.66      3.15
    ('bn', 'y'):                           4,    #   0.76      1.12
    ('bn', 'y eval'):                     15,    #   3.36      3.96
    ('stat_scalar', 'dbeta'):              4,    #   0.83      0.75
    ('stat_scalar', 'dgamma'):             2,    #   0.42      0.48
    ('bn', 'dx'):                         15,    #   3.59     19.85
    ('bn', 'acc_dgamma'):                  1,    #   0.15      0.15
    ('bn', 'acc_dbeta'):                   2,    #   0.50      0.58
    ('stat_vec', 'mean'):                 10,    #   2.50      1.98
    ('stat_vec', 'var'):                  25,    #   5.48      0.00
    ('stat_vec', 'run_mean'):              8,    #   1.95      2.50
    ('stat_vec', 'run_var'):              20,    #   3.82      1.94
    ('stat_vec', 'dbeta'):                15,    #   2.73      1.10
    ('stat_vec', 'dgamma'):                5,    #   1.08      0.51
    ('spade', 'out apply'):               15,    #   3.15      3.99
    ('spade', 'out'):                      1,    #   0.00      0.00
    ('spade', 'dz'):                       1,    #   0.00      0.59
    ('spade', 'dgamma'):                  15,    #   2.86      2.86
    ('spade_up2_onepass', 'dx'):           1,    #   0.00   4202.31
    ('spade_up2_onepass', 'dgamma'):      35,    #   8.03      2.55
    ('spade_up2_twopass', 'dx'):           1,    #   0.00   4624.20
    ('spade_up2_twopass', 'dgamma'):      35,    #   8.02      2.47
    ('spade_up2_fallback', 'dx'):          1,    #   0.00      0.00
    ('bil_fwd_x2', 'y'):                  10,    #   2.42      1.97
    ('bil_fwd_general', 'y'):              7,    #   1.67      1.96
    ('bil_bwd_x2', 'dx'):                 15,    #   2.57      2.57
    ('bil_bwd_general', 'dx'):             1,    #   0.00      0.00
    ('bil_bwd_tight3', 'dx'):              1,    #   0.00      0.00
    ('bil_bwd_tight5', 'dx'):              1,    #   0.00      0.00
    ('up2_stats', 'y'):                   10,    #   2.37      2.81
    ('up2_stats', 'mean'):                 5,    #   1.15      1.96
    ('up2_stats', 'var'):                  2,    #   0.41      0.00
    ('up2_stats_fallback', 'y'):          10,    #   2.31      2.37
    ('up2_stats_fallback', 'dx'):          8,    #   1.95      2.70
    # the sums of the SPADE backward passes stay in the workspace, so their kappa (what sums_propagated lets them move dz / dx by) cannot be measured:
    # 16, above the largest kappa an observable sum of the same kernels needed (d beta, 15), and the value the dz / dx margins above were measured under
    ('stat_scalar', 'sums'):              16,
    ('stat_vec', 'sums'):                 16,
    ('stat_interp', 'sums'):              16,    # the vector kernel's INTERP instantiation: the same loop and reduction
    ('spade_up2_onepass', 'sums'):        16,    # per-tile partial sums of <= 256 pixels over 8 (4) waves, combined in float64: shorter fp32 runs than the vector kernel's
}
