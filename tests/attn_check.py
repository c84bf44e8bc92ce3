"""Float64 references and error scales of the attention-decoder kernels (csrc/mrdis_outdec.hip: channel attention with the skip sum, symmetric
difference, residual gate) and of the latent-option kernels (csrc/mrdis_latent.hip: the masked KL term, the mean compaction); no GPU needed.

The bound is the one of tests/conv_check.py (check / ratio / U / TINY are its own, assert_same_bits is tests/elem_check.py's; imported, not copied):

    |got - ref| <= kappa * u * A  +  tiny          u = 2^-24

Every function returns (ref, A) in float64, or a dict of such pairs: ref from the fp32 operands the kernel actually reads, A the same expression on
the absolute value of every term.  Activations are NHWC: (B, HW, C) for the channel attention (its C ABI knows HW only), (B, H, W, C) elsewhere.

  * chatt forward, stage by stage, each stage from the STORED output of the stage in front of it (as the SPADE row of tests/test_gpu_conv_paths.py
    does with the statistics), so that one stage's rounding is not charged to the next:
        pool = mean_hw x                      A = mean_hw |x|
        hid  = relu(Wd pool + bd)             A = |Wd| |pool| + |bd|          (the ReLU applies to ref only: its slope is <= 1)
        a    = sigmoid(z), z = Wu hid + bu    A = a (1 - a) A_z + a           (aux_check.routing_ref's: what the rounding of z does to a, plus a's own)
        out  = (1 + a) x + s                  A = (1 + a) |x| + |s|
  * chatt backward from the a, hid, pool handed in: da = sum_hw dy x, dzu = da (1 - a) a, dWu = dzu^T hid, dbu = sum_b dzu,
    dzd = [hid > 0] dzu Wu, dWd = dzd^T pool, dbd = sum_b dzd, dpool = dzd Wd / HW, dx = (1 + a) dy + dpool; A the same chain on absolute values
    (a and (1 - a) a are positive).  The ReLU gate is read from the stored hid: no discontinuity enters.
  * symdiff: the forward is one subtraction and one abs, held to the bit (symdiff_fwd_bits).  The backward sgn(d) (dgd[h] + dgd[H-1-h]) has
    A = |dgd[h]| + |dgd[H-1-h]|; the sign of an fp32 difference is exact, so it is taken from the float64 difference of the fp32 inputs; sgn(0) = 0.
  * rgate: u = 1 + up2(alpha), up2 = F.interpolate(bilinear, align_corners=False) in float64; out = u x, A = (1 + up2(|alpha|)) |x|; dx likewise on
    dy; rsum = sum_c dy x, A = sum_c |dy| |x|; dalpha = up2^T rsum, A = up2^T A_rsum (the weights of up2 are >= 0).
  * KL (the two formulas of the header comment of csrc/mrdis_latent.hip).  A carries the conditioning of exp, which is its argument:
    e^lv (1 + |lv|), and (1 + |plv|) on everything divided by e^plv (the softmax row of tests/test_gpu_variants.py sets A this way); (m - pm)^2
    enters as (|m| + |pm|) |m - pm|.  The loss is one scalar, A = sum |w| (...); the gradients are element-wise, dpmu / dplv of a per-contrast
    prior summed over the batch, A likewise.  The upstream gradient g is a device scalar.
  * avgpool: F.avg_pool2d in float64, A the same on |x|; the backward is dy / k^2 (one rounding, A = |ref|) and exactly 0 in the floor remainder.

dtype=torch.float32 (the *_t functions): the same operation in plain fp32 torch on the CPU -- the yardstick KAPPA is set from
(tests/test_gpu_attn_paths.py TorchImpl)."""
import torch
import torch.nn.functional as F

from conv_check import U, TINY, check, ratio                         # noqa: F401  (re-exported: one bound for every table)
from elem_check import assert_same_bits                               # noqa: F401

F64 = torch.float64


# ---------------------------------------------------------------- channel attention.  x, s, dy (B, HW, C); wd (Hd, C), bd (Hd,), wu (C, Hd), bu (C,)
def chatt_pool_ref(x):
    x = x.double()
    return x.mean(1), x.abs().mean(1)


def chatt_hid_ref(pool, wd, bd):
    pool, wd, bd = pool.double(), wd.double(), bd.double()
    return F.relu(pool @ wd.T + bd), pool.abs() @ wd.abs().T + bd.abs()


def chatt_a_ref(hid, wu, bu):
    hid, wu, bu = hid.double(), wu.double(), bu.double()
    a = torch.sigmoid(hid @ wu.T + bu)
    Az = hid.abs() @ wu.abs().T + bu.abs()
    return a, a * (1 - a) * Az + a


def chatt_out_ref(x, s, a):
    x, s, g = x.double(), s.double(), 1 + a.double()[:, None, :]
    return g * x + s, g * x.abs() + s.abs()


def chatt_bwd_ref(dy, x, a, hid, pool, wd, wu):
    """-> dict(dx, dwd, dbd, dwu, dbu: (ref, A))"""
    dy, x, a, hid, pool, wd, wu = (t.double() for t in (dy, x, a, hid, pool, wd, wu))
    HW = x.shape[1]
    live = (hid > 0).double()
    g = (1 - a) * a
    out = []
    for absolute in (False, True):
        if absolute:
            dy_, x_, hid_, pool_, wd_, wu_ = (t.abs() for t in (dy, x, hid, pool, wd, wu))
        else:
            dy_, x_, hid_, pool_, wd_, wu_ = dy, x, hid, pool, wd, wu
        dzu = (dy_ * x_).sum(1) * g
        dzd = (dzu @ wu_) * live
        dpool = (dzd @ wd_) / HW
        out.append(dict(dx=(1 + a)[:, None, :] * dy_ + dpool[:, None, :], dwd=dzd.T @ pool_, dbd=dzd.sum(0), dwu=dzu.T @ hid_, dbu=dzu.sum(0)))
    return {k: (out[0][k], out[1][k]) for k in out[0]}


def chatt_fwd_t(x, s, wd, bd, wu, bu):
    """plain fp32 torch -> dict(out, pool, hid, a)"""
    pool = x.mean(1)
    hid = F.relu(pool @ wd.T + bd)
    a = torch.sigmoid(hid @ wu.T + bu)
    return dict(out=(1 + a)[:, None, :] * x + s, pool=pool, hid=hid, a=a)


def chatt_bwd_t(dy, x, a, hid, pool, wd, wu):
    dzu = (dy * x).sum(1) * (1 - a) * a
    dzd = (dzu @ wu) * (hid > 0).float()
    dpool = (dzd @ wd) / x.shape[1]
    return dict(dx=(1 + a)[:, None, :] * dy + dpool[:, None, :], dwd=dzd.T @ pool, dbd=dzd.sum(0), dwu=dzu.T @ hid, dbu=dzu.sum(0))


# ---------------------------------------------------------------- symmetric difference.  g, dgd (B, H, W, C)
def symdiff_fwd_bits(g):
    """fp32, exact: one IEEE subtraction, one abs"""
    return (g - g.flip(1)).abs()


def symdiff_bwd_ref(dgd, g):
    dgd, g = dgd.double(), g.double()
    return torch.sign(g - g.flip(1)) * (dgd + dgd.flip(1)), dgd.abs() + dgd.flip(1).abs()


# ---------------------------------------------------------------- residual gate.  x, dy (B, H, W, C), alpha (B, h, w), H = 2 h, W = 2 w
def up2(alpha):
    """(B, h, w) -> (B, 2 h, 2 w, 1), in alpha's dtype"""
    return F.interpolate(alpha[:, None], scale_factor=2, mode='bilinear', align_corners=False)[:, 0, :, :, None]


def up2_adjoint(r):
    """(B, H, W) float64 -> (B, H / 2, W / 2): the transpose of up2"""
    B, H, W = r.shape
    al = torch.zeros(B, H // 2, W // 2, dtype=r.dtype, requires_grad=True)
    return torch.autograd.grad((up2(al)[..., 0] * r).sum(), al)[0]


def rgate_fwd_ref(x, alpha):
    x, alpha = x.double(), alpha.double()
    return (1 + up2(alpha)) * x, (1 + up2(alpha.abs())) * x.abs()


def rgate_bwd_ref(dy, x, alpha):
    """-> dict(dx, rsum (B, H, W), dalpha (B, h, w): (ref, A))"""
    dy, x, alpha = dy.double(), x.double(), alpha.double()
    r, Ar = (dy * x).sum(3), (dy.abs() * x.abs()).sum(3)
    return dict(dx=((1 + up2(alpha)) * dy, (1 + up2(alpha.abs())) * dy.abs()), rsum=(r, Ar), dalpha=(up2_adjoint(r), up2_adjoint(Ar)))


def rgate_bwd_t(dy, x, alpha):
    """plain fp32 torch: autograd through (1 + up2(alpha)) x; rsum by its definition"""
    xr, ar = x.clone().requires_grad_(True), alpha.clone().requires_grad_(True)
    dx, dal = torch.autograd.grad(((1 + up2(ar)) * xr * dy).sum(), (xr, ar))
    return dict(dx=dx, rsum=(dy * x).sum(3), dalpha=dal)


# ---------------------------------------------------------------- KL.  mu, lv (M, B, Z); w (M, B); pm, plv None | (M, Z) | (M, B, Z); g a scalar
def _prior(pm, plv, dtype):
    if pm is None:
        return None, None
    pm, plv = pm.to(dtype), plv.to(dtype)
    return (pm[:, None], plv[:, None]) if pm.dim() == 2 else (pm, plv)


def kl_ref(mu, lv, w, pm=None, plv=None, g=1.0):
    """-> dict(loss (1,), dmu, dlv (M, B, Z) and, with a prior, dpmu, dplv of the prior's shape: (ref, A))"""
    mu, lv, w = mu.double(), lv.double(), w.double()
    row = pm is not None and pm.dim() == 2
    pm, plv = _prior(pm, plv, F64)
    gw, agw = (g * w)[:, :, None], (g * w).abs()[:, :, None]
    el, Ael = torch.exp(lv), torch.exp(lv) * (1 + lv.abs())
    if pm is None:
        kl, Akl = 0.5 * (el + mu * mu - 1 - lv), 0.5 * (Ael + mu * mu + 1 + lv.abs())
        out = dict(dmu=(gw * mu, agw * mu.abs()), dlv=(gw * 0.5 * (el - 1), agw * 0.5 * (Ael + 1)))
    else:
        d, ep, cp = mu - pm, torch.exp(plv), 1 + plv.abs()
        Ad2 = (mu.abs() + pm.abs()) * d.abs()
        kl = 0.5 * (-1 + (plv - lv) + (el + d * d) / ep)
        Akl = 0.5 * (1 + plv.abs() + lv.abs() + (Ael + Ad2) * cp / ep)
        dmu, Admu = gw * d / ep, agw * (mu.abs() + pm.abs()) * cp / ep
        dplv, Adplv = gw * 0.5 * (1 - (el + d * d) / ep), agw * 0.5 * (1 + (Ael + Ad2) * cp / ep)
        out = dict(dmu=(dmu, Admu), dlv=(gw * 0.5 * (-1 + el / ep), agw * 0.5 * (1 + Ael * cp / ep)))
        red = (lambda t: t.sum(1)) if row else (lambda t: t)
        out.update(dpmu=(red(-dmu), red(Admu)), dplv=(red(dplv), red(Adplv)))
    out['loss'] = ((w[:, :, None] * kl).sum().reshape(1), (w.abs()[:, :, None] * Akl).sum().reshape(1))
    return out


def kl_t(mu, lv, w, pm=None, plv=None, g=1.0):
    """plain fp32 torch: the reference's formula and autograd -> dict(loss, dmu, dlv[, dpmu, dplv])"""
    mu, lv = mu.clone().requires_grad_(True), lv.clone().requires_grad_(True)
    leaves = [mu, lv]
    if pm is None:
        kl = 0.5 * (torch.exp(lv) + mu ** 2 - 1 - lv)
    else:
        pm, plv = pm.clone().requires_grad_(True), plv.clone().requires_grad_(True)
        leaves += [pm, plv]
        p, q = _prior(pm, plv, torch.float32)
        kl = 0.5 * (-1 + (q - lv) + (torch.exp(lv) + (mu - p) ** 2) / torch.exp(q))
    loss = (kl.sum(2) * w).sum()
    grads = torch.autograd.grad(g * loss, leaves)
    return dict(zip(('dmu', 'dlv', 'dpmu', 'dplv'), grads), loss=loss.detach().reshape(1))


# ---------------------------------------------------------------- k x k mean pooling.  x (N, H, W, C) -> the compact vector (N, C * Ho * Wo)
def avgpool_ref(x, k):
    x = x.double().permute(0, 3, 1, 2)
    N = x.shape[0]
    return F.avg_pool2d(x, k).reshape(N, -1), F.avg_pool2d(x.abs(), k).reshape(N, -1)


def avgpool_bwd_ref(dy, shape, k):
    """dy (N, C * Ho * Wo), shape (N, H, W, C) -> dx (N, H, W, C): dy / k^2 under its window, 0 in the floor remainder"""
    N, H, W, C = shape
    Ho, Wo = H // k, W // k
    dx = torch.zeros(N, C, H, W, dtype=F64)
    dx[:, :, :Ho * k, :Wo * k] = (dy.double().reshape(N, C, Ho, Wo) / (k * k)).repeat_interleave(k, 2).repeat_interleave(k, 3)
    dx = dx.permute(0, 2, 3, 1).contiguous()
    return dx, dx.abs()


# kappa per (operation, output) of the rows of tests/test_gpu_attn_paths.py: 4 x the worst yardstick ratio SEEN over the operation's rows (the plain fp32
# torch evaluation on the CPU against the float64 reference; in the comment), rounded up, at least 1 -- NOT taken from the kernels under test.  fp32 torch
# rounds a little differently from CPU to CPU, so "seen" is the larger of the evaluations on record.
# profiles/attn_path_margins.txt lists its own run's yardstick beside this column and the kernels' ratio per row; tests/test_attn_check.py holds the
# table to the rows' yardsticks without a GPU.
# Summation orders of the kernels that differ from torch's (all inside their entries):
#   chatt pool and da (the partial sums of x and of dy x): a lane sums its pixels of a chunk in order, the lanes of a channel vector meet in order, then
#     the P chunks in order: at most ceil(chunk / npl) + npl + P terms in one fp32 chain -- 72 in the 1x1028x8x9 row, whose first channel group has
#     one lane per channel (npl = 1).  With B = 1 that row's dbu is da (1 - a) a itself and dWu that times hid: 3.5 - 3.8 against torch's cascaded
#     sum at 1.2 - 1.4 on the same row (profiles/attn_path_margins.txt), the widest gap of the table and inside the entries.
#   chatt_mlp_bwd sums sequentially: over b (B terms: up to 1025 in the B * CG > 1024 row) for dWu, dbu, dWd, dbd, over c (C terms: up to 1028)
#     for dzd and over j (Hd terms) for dpool, where torch's matmul and sum block their sums.
#   KL: the kernel adds the fp32 terms w * kl in double (the loss, dpmu, dplv): only the terms' own rounding and the final conversion remain.
KAPPA = {
    #                          kappa     yardstick
    ('chatt', 'pool'):             7,    #    1.70
    ('chatt', 'hid'):              9,    #    2.21
    ('chatt', 'a'):                8,    #    1.92
    ('chatt', 'out'):             11,    #    2.55
    ('chatt', 'dx'):              11,    #    2.52
    ('chatt', 'dwd'):              7,    #    1.72
    ('chatt', 'dbd'):              6,    #    1.40
    ('chatt', 'dwu'):              7,    #    1.75
    ('chatt', 'dbu'):              7,    #    1.53
    ('symdiff', 'dg'):             4,    #    1.00
    ('rgate', 'out'):             12,    #    2.86
    ('rgate', 'dx'):              12,    #    2.95
    ('rgate', 'rsum'):            12,    #    2.91
    ('rgate', 'dalpha'):           1,    #    0.24
    ('kl', 'loss'):                2,    #    0.39
    ('kl', 'dmu'):                10,    #    2.37
    ('kl', 'dlv'):                 6,    #    1.39
    ('kl', 'dpmu'):                6,    #    1.44
    ('kl', 'dplv'):                7,    #    1.61
    ('avgpool', 'y'):              9,    #    2.24
    ('avgpool', 'dx'):             1,    #    0.00
}
