"""Float64 references and error scales of the CondConv expert-mix kernels (csrc/mrdis_conv.hip), the optimizer arena and the helper kernels of
csrc/mrdis_elem.hip (softmax_mask_drop, recon_err, maxpool, cast_view, slice_gather); no GPU needed.

The bound is the one of tests/conv_check.py (check / ratio / U / TINY / bf16_round are its own, assert_same_bits is tests/elem_check.py's; imported,
not copied):

    |got - ref| <= kappa * u * A  +  u_out * |ref|  +  extra  +  tiny

Every function returns (ref, A) in float64 (or a dict of such pairs): ref from the operands the kernel actually reads -- the scalars of the C ABI
are floats, so lr, the betas, eps, the weight decay, max_norm and grad_scale enter the references as the float64 value of their fp32 rounding (f32())
-- and A the same expression on the absolute value of every term.  Per operation:

  * routing: r = sigmoid(z), z = fcw t_m + fcb.  A_r = r (1 - r) A_z + r: what the rounding of z (A_z = |fcw| |t| + |fcb|) does to r, plus r's own.
  * mixed filter: sum_e r[m][e] W[e], A = sum_e |r| |W[e]|.  End to end from the float64 r: the rounding of the routing is part of what kappa covers
    (the yardstick forms r in fp32 too).
  * dW[e] = sum_m r[m][e] dw_m over the types that have a gradient; A = sum_m |r[m][e]| |dw_m|.
  * dfcw, dfcb: float64 autograd through sum_m <dw_m, sum_e sigmoid(fcw t_m + fcb)[e] W[e]>.  A uses A_dr[m][e] = sum |dw_m| |W_e| times r (1 - r),
    times |t| for dfcw, summed over the types.  dr of the single-type entry point: A = |dr_0| + sum |dw| |W[e]| (it adds into dr).
  * Adam: torch.optim.Adam(amsgrad=True, weight_decay=wd, foreach=False) on float64 parameters, one parameter per gate range plus one for the ungated
    rest, grad = None where the range's flag is 0 (torch's per-parameter `step` then does the per-gate counting), the gradient scaled by grad_scale
    and clipped (clip_grad_norm_) in front of the step, the whole step skipped when a gradient element is non-finite.  A_p = |p| + K lr after K steps;
    A_m, A_v, A_vmax: the recurrences on absolute terms.
  * softmax with the dropped mask logit: F.softmax(cat([scale * mask, s]))[:, 1:] (mask None: plain softmax); the bound is relative to the element
    (A = ref) plus FLT_MIN (`extra`): outputs near e^-100 underflow in fp32 and not in float64.  Its backward from the STORED output:
    ds = o (d - sum o d), A = |o| (|d| + sum |o| |d|).
  * recon_err: per-sample mean of |d| or d^2, A the same; backward w[n] / (HW C) * sign(d) or * 2 d, A = |ref|.
  * maxpool, cast_view, slice_gather are exact: F.max_pool2d(return_indices=True), .to(dtype), an index-by-index gather on the host.

dtype=torch.float32 (adam_ref, softmax_md_ref, mix_routing_grad_ref): the same operation in plain fp32 torch on the CPU -- part of the yardstick KAPPA is
set from (tests/test_gpu_aux_paths.py TorchImpl)."""
import numpy as np
import torch
import torch.nn.functional as F

from conv_check import U, U_BF16, TINY, bf16_round, check, ratio      # noqa: F401  (re-exported: one bound for every table)
from elem_check import assert_same_bits                               # noqa: F401

FLT_MIN = 2.0 ** -126          # the smallest normal fp32


def f32(x):
    """the float64 value of a scalar as the C ABI passes it (fp32)"""
    return float(np.float32(x))


# ---------------------------------------------------------------- expert mixing.  W (E, Co, Ci, T); filters as (T, Ci, Co) [tck] | (T, Co, Ci) [tkc]
def to_tck(w):
    """(..., Co, Ci, T) -> (..., T, Ci, Co)"""
    return w.movedim(-1, -3).transpose(-1, -2).contiguous()


def to_tkc(w):
    """(..., Co, Ci, T) -> (..., T, Co, Ci)"""
    return w.movedim(-1, -3).contiguous()


def from_tck(g):
    """(..., T, Ci, Co) -> (..., Co, Ci, T)"""
    return g.transpose(-1, -2).movedim(-3, -1).contiguous()


def routing_ref(fcw, fcb, types):
    """fcw (E, emb), fcb (E,), types (M, emb) -> r (M, E), A_r"""
    fcw, fcb, types = fcw.double(), fcb.double(), types.double()
    z = types @ fcw.T + fcb
    Az = types.abs() @ fcw.abs().T + fcb.abs()
    r = torch.sigmoid(z)
    return r, r * (1 - r) * Az + r


def mix_fwd_ref(W, r):
    """W (E, Co, Ci, T), r (M, E) [or (E,)] -> mixed filters (M, Co, Ci, T) [(Co, Ci, T)], A = sum |r| |W|"""
    W, r = W.double(), r.double()
    return torch.einsum('...e,eoct->...oct', r, W), torch.einsum('...e,eoct->...oct', r.abs(), W.abs())


def mix_dW_ref(dws, r):
    """dws: M gradients (T, Ci, Co) or None, r (M, E) -> dW (E, Co, Ci, T), A = sum |r| |dw|"""
    r = r.double()
    A_r = r.abs()
    ref = A = 0
    for m, g in enumerate(dws):
        if g is None:
            continue
        g = from_tck(g.double())
        ref = ref + r[m][:, None, None, None] * g
        A = A + A_r[m][:, None, None, None] * g.abs()
    return ref, A


def mix_dr_ref(dw, W, dr0=None):
    """the single-type entry point: dr[e] = dr_0[e] + <dw, W[e]> -> (dr (E,), A)"""
    g, W = from_tck(dw.double()), W.double()
    ref, A = (g * W).sum((1, 2, 3)), (g.abs() * W.abs()).sum((1, 2, 3))
    if dr0 is not None:
        ref, A = ref + dr0.double(), A + dr0.double().abs()
    return ref, A


def mix_routing_grad_ref(W, fcw, fcb, types, dws, dtype=torch.float64):
    """autograd through the whole expression -> dict(dfcw=(ref, A), dfcb=(ref, A), dW=ref); dtype=torch.float32: the yardstick (A then meaningless)"""
    Wd, fw, fb = (x.detach().to(dtype).clone().requires_grad_(True) for x in (W, fcw, fcb))
    t = types.to(dtype)
    r = torch.sigmoid(t @ fw.T + fb)
    loss = 0
    for m, g in enumerate(dws):
        if g is not None:
            loss = loss + (torch.einsum('e,eoct->oct', r[m], Wd) * from_tck(g.to(dtype))).sum()
    if not torch.is_tensor(loss):          # no type has a gradient
        z = torch.zeros
        return dict(dfcw=(z(fcw.shape, dtype=dtype), z(fcw.shape, dtype=dtype)), dfcb=(z(fcb.shape, dtype=dtype), z(fcb.shape, dtype=dtype)), dW=z(W.shape, dtype=dtype))
    dW, dfw, dfb = torch.autograd.grad(loss, (Wd, fw, fb))
    rd = r.detach().double()
    A_b = torch.zeros(fcb.shape, dtype=torch.float64); A_w = torch.zeros(fcw.shape, dtype=torch.float64)
    for m, g in enumerate(dws):
        if g is not None:
            A_dr = (from_tck(g.double()).abs()[None] * W.double().abs()).sum((1, 2, 3)) * rd[m] * (1 - rd[m])
            A_b += A_dr; A_w += A_dr[:, None] * types[m].double().abs()[None]
    return dict(dfcw=(dfw.detach(), A_w), dfcb=(dfb.detach(), A_b), dW=dW.detach())


# ---------------------------------------------------------------- optimizer arena
def sumsq_ref(g, out0=(0.0, 0.0)):
    """-> (sum of squares of the finite elements + out0[0], its A (the sum itself), non-finite count + out0[1])"""
    g = g.double()
    fin = torch.isfinite(g)
    s = (g[fin] ** 2).sum() + out0[0]
    return s.reshape(1), s.reshape(1).clone(), int((~fin).sum()) + out0[1]


def adam_ref(p0, grads, flags, ranges, fidx, lr, b1, b2, eps, wd, max_norm, grad_scale=1.0, clip=True, dtype=torch.float64, arena_count=False):
    """K steps of the arena rule.  p0 (n,), grads: K tensors (n,) (zero where their range's flag is 0, as the arena holds them), flags: K lists of 0 / 1
    per flag (None: no gates), ranges [(lo, hi)], fidx [flag of range k]; clip False: no norm is given to the step (no clip, no skip).
    arena_count: every range is bias-corrected with the ARENA's count of applied steps (what the entry point does when it is given no gate_steps).
    -> dict(p, m, v, vmax: (ref, A) each (n,); applied, skipped, gate_steps [per flag])"""
    lr, b1, b2, eps, wd, max_norm, grad_scale = (f32(x) for x in (lr, b1, b2, eps, wd, max_norm, grad_scale))
    n = p0.numel()
    rest = torch.ones(n, dtype=torch.bool)
    segs = []
    for lo, hi in ranges:
        segs.append(torch.arange(lo, hi)); rest[lo:hi] = False
    segs.append(rest.nonzero().reshape(-1))
    seg_flag = list(fidx) + [None]
    params = [p0[i].to(dtype).clone().requires_grad_(True) for i in segs]
    live = [q for q in params if q.numel()]
    opt = torch.optim.Adam(live, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, amsgrad=True, foreach=False) if live else None
    if arena_count:          # the optimizer state as load_state_dict would leave it, so that `step` can be set from outside
        for q in live:
            opt.state[q] = dict(step=torch.tensor(0.0), exp_avg=torch.zeros_like(q), exp_avg_sq=torch.zeros_like(q), max_exp_avg_sq=torch.zeros_like(q))
    A_m = torch.zeros(n, dtype=torch.float64); A_v = torch.zeros(n, dtype=torch.float64); A_vm = torch.zeros(n, dtype=torch.float64)
    applied = skipped = 0
    n_flags = (max(fidx) + 1) if len(fidx) else 0
    gate_steps = [0] * n_flags
    for k, g in enumerate(grads):
        if clip and not bool(torch.isfinite(g).all()):
            skipped += 1
            continue
        applied += 1
        fl = flags[k] if flags is not None else None
        on = torch.zeros(n, dtype=torch.bool)
        for q, i, f in zip(params, segs, seg_flag):
            live_ = f is None or fl is None or fl[f] != 0
            q.grad = (g[i].to(dtype) * grad_scale) if (live_ and q.numel()) else None
            if live_:
                on[i] = True
        if fl is not None:
            for f in range(n_flags):
                gate_steps[f] += int(fl[f] != 0)
        gs = [q for q in live if q.grad is not None]
        coef = grad_scale
        if clip and max_norm > 0 and gs:
            tn = torch.nn.utils.clip_grad_norm_(gs, max_norm, foreach=False)
            coef = grad_scale * min(1.0, max_norm / (float(tn) + 1e-6))
        pa = torch.zeros(n, dtype=torch.float64)
        for q, i in zip(params, segs):
            pa[i] = q.detach().double().abs()
        ga = torch.where(on, g.double().abs() * coef + wd * pa, torch.zeros(n, dtype=torch.float64))
        A_m = torch.where(on, b1 * A_m + (1 - b1) * ga, A_m)
        A_v = torch.where(on, b2 * A_v + (1 - b2) * ga * ga, A_v)
        A_vm = torch.maximum(A_vm, A_v)
        if arena_count:
            for q in gs:
                opt.state[q]['step'].fill_(applied - 1)
        if gs:
            opt.step()
    out = {name: torch.zeros(n, dtype=torch.float64) for name in ('p', 'm', 'v', 'vmax')}
    for q, i in zip(params, segs):
        st = opt.state.get(q, {}) if opt is not None else {}
        out['p'][i] = q.detach().double()
        for name, key in (('m', 'exp_avg'), ('v', 'exp_avg_sq'), ('vmax', 'max_exp_avg_sq')):
            if key in st:
                out[name][i] = st[key].double()
    K = len(grads)
    return dict(p=(out['p'], out['p'].abs() + K * lr), m=(out['m'], A_m), v=(out['v'], A_v), vmax=(out['vmax'], A_vm),
                applied=applied, skipped=skipped, gate_steps=gate_steps)


# ---------------------------------------------------------------- helpers
def softmax_md_ref(s, mask, scale=100.0, dtype=torch.float64):
    """s (P, C), mask (P,) or None -> (ref (P, C), A = ref, extra = FLT_MIN)"""
    s = s.to(dtype)
    if mask is None:
        out = F.softmax(s, 1)
    else:
        out = F.softmax(torch.cat([f32(scale) * mask.to(dtype)[:, None], s], 1), 1)[:, 1:]
    return out, out.clone(), torch.full(out.shape, FLT_MIN, dtype=torch.float64)


def softmax_md_bwd_ref(dout, out):
    """from the stored output: ds = o (d - sum_c o d)"""
    d, o = dout.double(), out.double()
    return o * (d - (o * d).sum(1, keepdim=True)), o.abs() * (d.abs() + (o.abs() * d.abs()).sum(1, keepdim=True))


def recon_err_ref(gt, x, p):
    """gt, x (N, ...) -> per-sample mean of |gt - x| (p = 1) or its square (p = 2); every term is >= 0: A = ref"""
    d = (gt.double() - x.double()).reshape(gt.shape[0], -1)
    e = d.abs().mean(1) if p == 1 else (d * d).mean(1)
    return e, e.clone()


def recon_err_bwd_ref(gt, x, w, p):
    d = x.double() - gt.double()
    cnt = d[0].numel()
    wv = w.double().reshape((-1,) + (1,) * (d.dim() - 1)) / cnt
    ref = wv * (torch.sign(d) if p == 1 else 2 * d)
    return ref, ref.abs()


def maxpool_ref(x, k):
    """x (N, C, H, W) fp32 -> (y, argmax as h * W + w, int32): exact, the first maximum in scan order wins, NaN propagates"""
    y, idx = F.max_pool2d(x, k, return_indices=True)
    return y, idx.to(torch.int32)


def maxpool_bwd_ref(dy, arg, in_shape):
    N, C, H, W = in_shape
    dx = torch.zeros(N, C, H * W, dtype=dy.dtype)
    dx.scatter_(2, arg.long().reshape(N, C, -1), dy.reshape(N, C, -1))
    return dx.reshape(N, C, H, W)


def cast_view_ref(x, dtype, Cd):
    """x (N, C, H, W) fp32 | bf16 -> (N, Cd, H, W) of `dtype`: the first min(C, Cd) channels converted (round to nearest even), the rest zero"""
    N, C, H, W = x.shape
    y = torch.zeros(N, Cd, H, W, dtype=dtype)
    c = min(C, Cd)
    y[:, :c] = x[:, :c].to(dtype)
    return y


def slice_gather_ref(vols, slice_idx, drop, H, W, D, block):
    """vols[b][m]: (D, H, W) fp32 or None -> inputs (B, M (2 block + 1), H, W), mask (B, M), mask_img (B, H, W); index by index"""
    B, M, c7 = len(vols), len(vols[0]), 2 * block + 1
    inputs = torch.zeros(B, M * c7, H, W); mask = torch.zeros(B, M)
    for b in range(B):
        for m in range(M):
            v = vols[b][m]
            live = v is not None and m != int(drop[b])
            mask[b, m] = 1.0 if live else 0.0
            for k in range(c7):
                sk = int(slice_idx[b]) - block + k
                if live and 0 <= sk < D:
                    inputs[b, m * c7 + k] = v[sk]
    return inputs, mask, (inputs[:, 0] == 0).float()


# kappa per (operation, output) of the rows of tests/test_gpu_aux_paths.py: 4 x the worst yardstick ratio SEEN over the operation's rows (the plain fp32
# torch evaluation on the CPU against the float64 reference; in the comment), rounded up, at least 1 -- NOT taken from the kernels under test.  fp32 torch
# rounds a little differently from CPU to CPU, so "seen" is the larger of the evaluations on record: profiles/aux_path_margins.txt lists its own run's
# yardstick beside this column and the kernels' ratio per row; tests/test_aux_check.py holds the table to the rows' yardsticks without a GPU.
# The softmax forms l - max in fp32 before the exponential: at logits of +-80 beside a mask logit of 100 that rounding alone is up to 180 u relative to
# the element, in torch and in the kernel alike -- hence the one large entry.
KAPPA = {
    #                          kappa     yardstick
    ('mix', 'r'):                  5,    #    1.21
    ('mix', 'w'):                 14,    #    3.38
    ('mix', 'dW'):                14,    #    3.43
    ('mix', 'dfcw'):               3,    #    0.57
    ('mix', 'dfcb'):               3,    #    0.50
    ('mix1', 'w'):                 9,    #    2.25
    ('mix1', 'dW'):                4,    #    0.98
    ('mix1', 'dr'):                2,    #    0.34
    ('sumsq', 'sum'):              5,    #    1.12
    ('adam', 'p'):                14,    #    3.45
    ('adam', 'm'):                16,    #    3.87
    ('adam', 'v'):                37,    #    9.14
    ('adam', 'vmax'):             37,    #    9.14
    ('softmax', 'out'):          139,    #   34.68
    ('softmax', 'ds'):            14,    #    3.41
    ('recon', 'err'):             15,    #    3.67
    ('recon', 'dx'):              12,    #    2.85
}
