"""Float64 references, error scales and the row tables of the 3-D GroupNorm(+ReLU) and nearest x2-upsampling kernels (csrc/mrdis_elem3d.hip); no
GPU needed.

The bound is the one of tests/conv_check.py (check / ratio / U / TINY are its own) and the column-statistics, apply and backward references are
those of tests/elem_check.py, imported and not copied: a GroupNorm over (N, C, D, H, W) with G groups is column statistics over the regrouping
(N G, 1, C / G, P) -- N G sample blocks of one "channel" each, whose "pixels" are the C / G channels x P voxels of the group (_rg).

    |got - ref| <= kappa * u * A  +  extra  +  tiny                   (fp32 throughout: no u_out)

Tensors are logical (N, C, D, H, W); statistics are (N G,), sample-major, as the kernels store them.  Per operation:

  * statistics: mean has A = mean|x|; the kernel returns rstd, the variance is recovered as 1 / rstd^2 - eps (var_from_rstd) and checked against the
    two-pass float64 variance with A_var = mean(x^2) + mean^2, the honest scale of the kernel's ONE-PASS E[x^2] - mean^2 from fp32 chunk partials
    (a mean 30 sigma from zero makes A_var 1800 x the variance, and the bound says so), plus rstd_rounding.
  * apply: (x - m) rstd gamma + beta, A = (|x| + |m|) rstd |gamma| + |beta|.  Checked against the statistics THE KERNEL RETURNED ('y apply': a
    fault is then the apply kernel's) and end to end against float64 statistics with their own bound propagated ('y', gn_stats_propagated).
    ReLU: ref = max(z, 0), A unchanged.  max(., 0) is 1-Lipschitz, so an element whose float64 pre-activation z lies within its own bound of 0
    may come back as 0 or as z without a special case.
  * backward: dz = dy [y > 0] with the mask taken from the y THE FORWARD STORED for the same row -- the backward recomputes it from x and must agree
    with the forward it belongs to.  S1 = sum_p dz, S2 = sum_p dz xhat per (n, c); d beta_c = sum_n S1, d gamma_c = sum_n S2, A the sum of the
    absolute terms.  dx = rstd (dz gamma - c1 - xhat c2), c1 | c2 = sum_{c in g} gamma_c S1 | S2 / (P C / G), formed term by term from float64 sums;
    what the sums' own bound allows comes back as `extra` (sums_propagated).
    An element is AMBIGUOUS when its float64 |z| (from the statistics the kernel returned) is within the apply bound kappa u A of 0: fp32 may put
    it on either side.  It may take either mask in dx (extra: its own term rstd |dy gamma|), and it adds |dy| to the extra of its S1 and |dy xhat|
    to the extra of its S2 (and through them to d beta, d gamma, c1, c2).  Outside the ambiguous elements the stored mask must equal [z > 0]
    (`mask_disagree`).  The share of ambiguous elements is capped at AMBIGUOUS_CAP: a condition of the rows' inputs that the tests assert
    (tests/test_elem3d_check.py evaluates it for every row from the float64 reference alone), not a tolerance.
  * x2 upsampling: an index copy (+ skip: one fp32 rounding) and an 8-term sum in the kernel's documented order (depth offset, then height, then
    width, from 0.f): both are held to the BITS of the same fp32 expression evaluated by torch on the CPU, and take no kappa.

The rows of tests/test_gpu_elem3d_paths.py and their seeded input builders live here so that tests/test_elem3d_check.py can evaluate the
conditions the rows rely on (the ambiguous share) without a GPU."""
import torch

from conv_check import U, TINY, check, ratio                      # noqa: F401  (re-exported: one bound for every table)
from elem_check import (stats_ref, var_from_rstd, rstd_rounding, norm_apply_ref, stats_propagated, bwd_sums_ref, bwd_apply_ref,      # noqa: F401
                        sums_propagated, assert_same_bits)

EPS = 1e-5
AMBIGUOUS_CAP = 1e-3


# ---------------------------------------------------------------- GroupNorm
def _rg(t, G):
    """(N, C, D, H, W) -> (N G, 1, C / G, P): elem_check's layout with one sample block per (n, g)"""
    N, C = t.shape[:2]
    assert C % G == 0
    return t.double().reshape(N * G, 1, C // G, -1)


def _chan(v, x):
    return v.detach().double().cpu().reshape(1, -1, 1, 1, 1) + 0 * x.double()


def groups_of(stat, x):
    return stat.numel() // x.shape[0]


def gn_stats_ref(x, G, eps=EPS):
    """-> {mean: (ref, A), var: (ref, A), rstd: ref, P: values per group}; all (N G,); the variance two-pass in float64"""
    return stats_ref(_rg(x, G), x.shape[0] * G, eps)


def gn_apply_ref(x, mean, rstd, gamma, beta, relu):
    """(ref, A, z): z = (x - m) rstd gamma + beta with the statistics as given ((N G,)), ref = max(z, 0) with ReLU"""
    G = groups_of(mean, x)
    xh, Ah = norm_apply_ref(_rg(x, G), mean, rstd, x.shape[0] * G)
    g, b = _chan(gamma, x), _chan(beta, x)
    z = xh.reshape(x.shape) * g + b
    return (z.clamp_min(0) if relu else z), Ah.reshape(x.shape) * g.abs() + b.abs(), z


def gn_stats_propagated(x, st, gamma, k_mean, k_var, eps=EPS):
    """the `extra` of the end-to-end check of y: what statistics inside their own bound move it by"""
    G = groups_of(st['rstd'], x)
    return stats_propagated(_rg(x, G), st, x.shape[0] * G, _rg(_chan(gamma, x), G), k_mean, k_var, eps).reshape(x.shape)


def gn_ambiguous(z, A, k_apply, relu=True):
    """the elements whose ReLU mask fp32 may decide either way: float64 |z| within the apply bound of 0"""
    return (z.abs() <= k_apply * U * A + TINY) if relu else torch.zeros_like(z, dtype=torch.bool)


def gn_bwd_ref(dy, x, gamma, beta, mean, rstd, G, relu, mask=None, k_apply=0.0, k_sum=0.0):
    """mask: y_kernel > 0 of the same row (None: the float64 [z > 0]) -> {dbeta | dgamma | dx: (ref, A, extra), share, mask_disagree}"""
    N, C = x.shape[:2]
    cg, P = C // G, x[0, 0].numel()
    m = P * cg
    _, A_z, z = gn_apply_ref(x, mean, rstd, gamma, beta, relu)
    amb = gn_ambiguous(z, A_z, k_apply, bool(relu))
    own = z > 0
    mask = own if mask is None else mask.detach().cpu().bool()
    disagree = int(((mask != own) & ~amb).sum()) if relu else 0
    dy = dy.double()
    dz = dy * mask if relu else dy
    # per (n, c): elem_check's sums with one sample block per (n, c)
    per_nc = lambda s: s.detach().double().cpu().reshape(N, G, 1).expand(N, G, cg).reshape(-1)
    nc = lambda t: t.double().reshape(N * C, 1, 1, P)
    S1, A1, S2, A2 = bwd_sums_ref(nc(dz), nc(x), per_nc(mean), per_nc(rstd), N * C)
    xh = (_rg(x, G) - mean.detach().double().cpu().reshape(-1, 1, 1, 1)) * rstd.detach().double().cpu().reshape(-1, 1, 1, 1)
    E1 = nc(dy.abs() * amb).sum((1, 2, 3))
    E2 = nc((dy * xh.reshape(x.shape)).abs() * amb).sum((1, 2, 3))
    over_n = lambda t: t.reshape(N, C).sum(0)
    g64 = gamma.detach().double().cpu()
    over_c = lambda t, w: (t.reshape(N, C) * w).reshape(N, G, cg).sum(2).reshape(-1)
    s0, s1 = over_c(S1, g64), over_c(S2, g64)
    A0g, A1g, E0g, E1g = (over_c(t, g64.abs()) for t in (A1, A2, E1, E2))
    gx = _rg(x, G)
    ref, A = bwd_apply_ref(_rg(dz * _chan(gamma, x), G), gx, mean, rstd, N * G, s0, s1, m)
    extra = sums_propagated(gx, mean, rstd, N * G, A0g, A1g, m, k_sum) + sums_propagated(gx, mean, rstd, N * G, E0g, E1g, m, 1.0 / U)
    r = rstd.detach().double().cpu().reshape(N, G, 1).expand(N, G, cg).reshape(N, C, 1, 1, 1)
    extra = extra.reshape(x.shape) + amb * r * (dy * _chan(gamma, x)).abs()
    return dict(dbeta=(over_n(S1), over_n(A1), over_n(E1)), dgamma=(over_n(S2), over_n(A2), over_n(E2)),
                dx=(ref.reshape(x.shape), A.reshape(x.shape), extra), share=float(amb.double().mean()), mask_disagree=disagree)


# ---------------------------------------------------------------- nearest x2 upsampling
def up2_ref(x, skip=None):
    """x (N, C, D, H, W) -> x[d / 2, h / 2, w / 2] (+ skip) in x's own dtype: an index copy and at most one rounding"""
    y = x.repeat_interleave(2, 2).repeat_interleave(2, 3).repeat_interleave(2, 4)
    return y if skip is None else y + skip


def up2_bwd_ref(dy):
    """the 8 children of each voxel summed one after the other in dy's own dtype, in the kernel's order: depth offset, then height, then width, from 0"""
    N, C, D2, H2, W2 = dy.shape
    a = torch.zeros((N, C, D2 // 2, H2 // 2, W2 // 2), dtype=dy.dtype)
    for kd in (0, 1):
        for kh in (0, 1):
            for kw in (0, 1):
                a = a + dy[:, :, kd::2, kh::2, kw::2]
    return a


# ---------------------------------------------------------------- the rows of tests/test_gpu_elem3d_paths.py and their inputs
def _gn(rid, N, C, dhw, G, relu=1, mean=0.5):
    return dict(id=rid, N=N, C=C, dhw=tuple(dhw), G=G, relu=relu, mean=mean)


GN_ROWS = [
    _gn('P2047 G=C last chunk one row short', 1, 8, (1, 1, 2047), 8),
    _gn('P2048 G=C one full chunk', 1, 8, (1, 1, 2048), 8),
    _gn('P2049 G=C one-row last chunk', 1, 8, (1, 1, 2049), 8),
    _gn('C4 G1 P131073 65 chunks', 1, 4, (1, 1, 131073), 1),
    _gn('C4 G2 P1025 one-row last block', 1, 4, (1, 1, 1025), 2),
    _gn('N3 C16 ragged grid', 3, 16, (5, 7, 9), 8),
    _gn('C64 G2 eight quads per group', 2, 64, (3, 5, 7), 2),
    _gn('C256 four rows per pass', 2, 256, (1, 3, 5), 8),
    _gn('C512 two rows per pass', 2, 512, (1, 3, 5), 8),
    _gn('C1024 one row per pass', 2, 1024, (1, 3, 5), 8),
    _gn('P1 C32', 2, 32, (1, 1, 1), 8),
    _gn('C64 no ReLU', 1, 64, (3, 5, 7), 8, relu=0),
    _gn('C32 mean 30 sigma', 1, 32, (9, 16, 16), 8, mean=30.0),
]


def _up(rid, N, C, D, H, W, what=('fwd', 'fwd_skip', 'bwd'), ints=False):
    return dict(id=rid, geom=(N, C, D, H, W), what=tuple(what), ints=ints)


UP_ROWS = [
    _up('N2 C16 3x5x4', 2, 16, 3, 5, 4),
    _up('C4 1x1x1', 1, 4, 1, 1, 1),
    _up('N2 C8 1x7x1', 2, 8, 1, 7, 1),
    _up('C12 5x1x3', 1, 12, 5, 1, 3),
    _up('C256 9x32x32 forward over the block cap', 1, 256, 9, 32, 32, what=('fwd_skip',)),
    _up('C1024 17x31x32 backward over the block cap', 1, 1024, 17, 31, 32, what=('bwd',), ints=True),
]


def rnd(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def data(shape, seed, mean=0.5):
    """seeded normal, sigma 2 around `mean`; unit sigma around a far mean"""
    return rnd(shape, seed, 2.0 if abs(mean) < 10 else 1.0) + mean


def gn_inputs(row):
    """fp32 on the host: x, dy, add (N, C, D, H, W); gamma = 1 + 0.3 randn, beta = 0.2 randn (C,)"""
    shape = (row['N'], row['C']) + row['dhw']
    C = row['C']
    return dict(x=data(shape, 1, row['mean']), dy=data(shape, 2), add=data(shape, 3), gamma=1.0 + rnd((C,), 4, 0.3), beta=rnd((C,), 5, 0.2))


# kappa per output of the GroupNorm rows of tests/test_gpu_elem3d_paths.py: about 4x the worst measured ratio (in the comment, with the ratio of a
# plain fp32 torch evaluation on the CPU against the same float64 reference -- the yardstick -- after it; profiles/elem3d_path_margins.txt), at least 1.
# More than 4x above the yardstick of their own row measure only (profiles/elem3d_path_margins.txt has the rows' numbers):
#   * the variances (4.76 against 0.00): the kernel forms E[x^2] - mean^2 in one pass from fp32 chunk partials, torch's var makes two passes -- the
#     documented cost that A_var = mean(x^2) + mean^2 is there to absorb (the mean-30-sigma row, A_var = 1800 var, measures 1.33);
#   * d beta / d gamma (and, just under 4x, the mean) of the C = 4 and C = 8 rows with one or two chunks (2.44 against 0.46): with C / 4 = 1 or 2 quads a block
#     has 256 or 128 row lanes, which gn_partial_kernel folds one after the other in fp32 (the fixed order that makes the result reproducible); torch's
#     sum is pairwise.  The same order emulated in fp32 on the CPU gives the same d beta ratios to the digit (1.55 | 1.44 | 2.40 | 0.16 | 2.44), and
#     the 65-chunk row, whose chunks are combined in double, measures 0.16.
# 'sums' is what sums_propagated lets the per-(n, c) sums move dx by.  With N = 1 they ARE d beta / d gamma, so they take those outputs' kappa.
# A measured value near 0 ('y') means the row's `extra` (the statistics' own bound propagated) already covers the error.
KAPPA = {
    #                    kappa     measured  yardstick
    ('gn', 'mean'):        8,    #   1.77      1.54
    ('gn', 'var'):        20,    #   4.76      0.00
    ('gn', 'y apply'):    10,    #   2.27      2.87
    ('gn', 'y'):           2,    #   0.29      0.64
    ('gn', 'dbeta'):      10,    #   2.44      1.54
    ('gn', 'dgamma'):     10,    #   2.43      1.43
    ('gn', 'dx'):          6,    #   1.47      1.52
    ('gn', 'sums'):       10,
}
