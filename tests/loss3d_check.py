"""Float64 references and error scales of the fused 3-D objective and of the segmentation counts (csrc/mrdis_loss3d.hip: mrdis_nvnet_loss_fwd / _bwd,
mrdis_seg_counts), and the rows of tests/test_gpu_loss3d_paths.py as geometry plus seed; no GPU needed.

The bound is the one of tests/conv_check.py (check / ratio / U / TINY are its own, assert_same_bits is tests/elem_check.py's; imported, not copied):

    |got - ref| <= kappa * u * A  +  tiny          u = 2^-24

Every function returns (ref, A) in float64, or a dict of such pairs: ref from the fp32 operands the kernel reads, A the per-element error scale.

  * sums = [A0, P2, T2, SE] = [sum p t, sum p^2, sum t^2, sum (v - x)^2], p the float64 sigmoid.  Every term is non-negative, so the sums on absolute
    values are the sums themselves: A = ref.
  * terms, each from the sums THE IMPLEMENTATION STORED (stage by stage, as attn_check does with pool / hid / a), so that the sums' own rounding is not
    charged a second time:   den = P2 + T2 + 1e-6
        dice = 1 - 2 A0 / den           A = 1 + 2 A0 / den
        l2   = SE / n2  (0 for n2 = 0)  A = ref
        obj  = dice + w_l2 l2           A = A_dice + |w_l2| A_l2
  * du = g (c1 t + c2 p) p (1 - p), c1 = -2 / den, c2 = 4 A0 / den^2 from the stored sums.  The kernel's stated numerics are "p is the fp32 sigmoid":
    p carries one fp32 rounding, dp = u p, before anything else is formed.  With q(p) = p (1 - p), dq / dp = 1 - 2 p: that rounding moves q by
    |1 - 2 p| p u -- next to q itself that is nothing at p = 1/2 and everything as p -> 1, where q -> 0 while p |1 - 2 p| -> 1 (beyond u ~ 17 the
    fp32 p IS 1 and du is exactly 0).  The same rounding moves c2 p by |c2| p u.  The roundings of the products and of the stored fp32 result are
    relative to the terms: (|c1| t + |c2| p) q.  Together
        A = |g| [ (|c1| t + |c2| p) (p (1 - p) + p |1 - 2 p|)  +  |c2| p * p (1 - p) ]
    On the t = 1 voxels c1 t and c2 p have opposite signs and cancel; A carries their magnitudes, not their difference.
  * dv = g w_l2 2 (v - x) / n2, A = |ref|: the difference of two fp32 values is exact in fp64, every later operation is a product.
  * seg counts: exact integers from the float64 sigmoid, with a mask of EXCUSED voxels whose side of the threshold an fp32 sigmoid may legitimately
    decide either way: |u| < 1e-6 for logits, |p - 0.5| < 1e-6 for probabilities.  u == 0 and p == 0.5 exactly are NOT excused: sigmoid(0) is 0.5 in
    any precision and 0.5 is not above 0.5.  The device counts must lie between the counts without and with the excused voxels.

The *_t functions are the same operations in plain torch on the CPU -- the yardsticks KAPPA is set from.  terms / du / dv: model3d.nvnet_loss's formula
(the KL term aside; w_l2 in place of its 0.1; mean written as sum / n so that the sum it divides is on record) in fp32 with autograd.  sums: fp32
torch.sigmoid, products and sums in float64 -- the kernel's stated numerics restated on the host; a pure fp32 torch sum would set the sums' kappa by
torch's own summation error (1e3 u at these sizes) and a dropped tail would pass under it."""
import functools
import os
import re

import torch

from conv_check import U, TINY, check, ratio                         # noqa: F401  (re-exported: one bound for every table)
from elem_check import assert_same_bits                               # noqa: F401

F64 = torch.float64
DICE_EPS = 1e-6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, 'representation-disentanglement_amd', 'csrc', 'mrdis_loss3d.hip')


def source_constants():
    """(L3_THREADS, L3_MAX_BLOCKS, L3_UNROLL) as csrc/mrdis_loss3d.hip states them"""
    src = open(SOURCE).read()
    return tuple(int(re.search(r'constexpr int %s = (\d+);' % name, src).group(1)) for name in ('L3_THREADS', 'L3_MAX_BLOCKS', 'L3_UNROLL'))


L3_THREADS, L3_MAX_BLOCKS, L3_UNROLL = source_constants()
T_CAP = L3_MAX_BLOCKS * L3_THREADS          # threads of a capped grid: the T of the row table
UN = L3_UNROLL                              # (U is the unit roundoff)


# ---------------------------------------------------------------- the source's launch geometry, restated
def l3_blocks(n1, n2):
    nv = max(n1, n2) >> 2
    return max(1, min(L3_MAX_BLOCKS, -(-nv // L3_THREADS)))


def stream_phases(n, threads):
    """what l3_stream does with n floats on a launch of `threads` threads: dict(body: threads that take the unrolled body at least once, body_max: the
    most iterations one takes, rem: threads that take the remainder loop at least once, rem_max, tail: n % 4, threads)"""
    nv = n >> 2
    tid = torch.arange(threads, dtype=torch.int64)
    step = UN * threads
    m = torch.clamp((nv - (UN - 1) * threads - tid + step - 1) // step, min=0)          # body iterations: i = tid + k step while i + (UN - 1) T < nv
    r = torch.clamp((nv - (tid + m * step) + threads - 1) // threads, min=0)            # remainder iterations from where the body stopped
    return dict(body=int((m > 0).sum()), body_max=int(m.max()), rem=int((r > 0).sum()), rem_max=int(r.max()), tail=n & 3, threads=threads)


def phase_name(ph):
    """(body taken, 'zero' | 'partial' | 'all' threads in the remainder, tail)"""
    return ph['body'] > 0, 'zero' if ph['rem'] == 0 else ('all' if ph['rem'] == ph['threads'] else 'partial'), ph['tail']


def shape5(n):
    """a 5-D shape of n elements: the prime factors of n dealt out over (B, C, D, H, W), largest first onto the smallest extent; a count with fewer
    than five factors leaves extents of 1"""
    if n == 0:
        return None
    f, k, d = [], n, 2
    while d * d <= k:
        while k % d == 0:
            f.append(d); k //= d
        d += 1
    if k > 1:
        f.append(k)
    dims = [1] * 5
    for p in sorted(f, reverse=True):
        dims[dims.index(min(dims))] *= p
    return tuple(dims)


def f32(g):
    """the value an fp32 scalar holds: the upstream gradient reaches the kernel (and autograd) as one fp32 value on the device"""
    return float(torch.tensor(g, dtype=torch.float32))


# ---------------------------------------------------------------- objective: float64
def sums_ref(u, t, v=None, x=None):
    p, td = torch.sigmoid(u.double()), t.double()
    se = ((v.double() - x.double()) ** 2).sum() if v is not None else torch.zeros((), dtype=F64)
    ref = torch.stack([(p * td).sum(), (p * p).sum(), (td * td).sum(), se])
    return ref, ref.clone()


def _coef(sums):
    a0, p2, t2, se = (float(s) for s in sums.double())
    den = p2 + t2 + DICE_EPS
    return a0, den, se


def terms_ref(sums, n2, w_l2):
    """-> dict(dice, l2, obj: (ref (1,), A (1,))) from the sums handed in"""
    a0, den, se = _coef(sums)
    q = 2.0 * a0 / den
    l2 = se / n2 if n2 > 0 else 0.0
    one = lambda a: torch.tensor([a], dtype=F64)
    return dict(dice=(one(1.0 - q), one(1.0 + q)), l2=(one(l2), one(l2)), obj=(one(1.0 - q + w_l2 * l2), one(1.0 + q + abs(w_l2) * l2)))


def du_ref(u, t, sums, g=1.0):
    """see the module docstring for A"""
    a0, den, _ = _coef(sums)
    c1, c2 = -2.0 / den, 4.0 * a0 / (den * den)
    p, td = torch.sigmoid(u.double()), t.double()
    q = p * (1 - p)
    lin = abs(c1) * td.abs() + abs(c2) * p
    return g * (c1 * td + c2 * p) * q, abs(g) * (lin * (q + p * (1 - 2 * p).abs()) + abs(c2) * p * q)


def dv_ref(v, x, g, w_l2):
    ref = (g * w_l2 * 2.0 / v.numel()) * (v.double() - x.double())
    return ref, ref.abs()


# ---------------------------------------------------------------- objective: the yardsticks
def sums_t(u, t, v=None, x=None):
    """the kernel's stated numerics on the host: the fp32 sigmoid torch computes, products and sums in float64"""
    p, td = torch.sigmoid(u).double(), t.double()
    se = ((v.double() - x.double()) ** 2).sum() if v is not None else torch.zeros((), dtype=F64)
    return torch.stack([(p * td).sum(), (p * p).sum(), (td * td).sum(), se])


def objective_t(u, t, v, x, w_l2, g):
    """nvnet_loss's formula in fp32 with autograd -> dict(stored: the four fp32 sums the formula divided (float64 tensor), terms (3,), du, dv | None)"""
    ur = u.clone().requires_grad_(True)
    p = torch.sigmoid(ur)
    a0, p2, t2 = (p * t).sum(), (p * p).sum(), (t * t).sum()
    dice = 1 - 2 * a0 / (p2 + t2 + DICE_EPS)
    leaves = [ur]
    if v is not None:
        vr = v.clone().requires_grad_(True)
        leaves.append(vr)
        se = ((vr - x) ** 2).sum()
        l2 = se / v.numel()
    else:
        se = l2 = torch.zeros(())
    obj = dice + w_l2 * l2
    grads = torch.autograd.grad(g * obj, leaves)
    return dict(stored=torch.stack([a0, p2, t2, se]).detach().double(), terms=torch.stack([dice, l2, obj]).detach(), du=grads[0], dv=grads[1] if v is not None else None)


# ---------------------------------------------------------------- segmentation counts.  pred, target (B, P, C): the memory order of channels-last-3d
EXCUSE = 1e-6


def seg_counts_ref(pred, target, logits):
    """-> (counts (B, C, 3) int64 = [|predicted and labelled|, |predicted|, |labelled|] from the float64 sigmoid, excused (B, P, C) bool)"""
    x = pred.double()
    p = torch.sigmoid(x) if logits else x
    centre = 0.0 if logits else 0.5
    excused = ((x - centre).abs() < EXCUSE) & (x != centre)
    pp, tt = p > 0.5, target == 1
    return torch.stack([(pp & tt).sum(1), pp.sum(1), tt.sum(1)], -1), excused


def seg_counts_bounds(pred, target, logits):
    """-> (lo, hi) (B, C, 3) int64: the counts with every excused voxel taken as not predicted / as predicted"""
    x = pred.double()
    pp = (torch.sigmoid(x) if logits else x) > 0.5
    _, excused = seg_counts_ref(pred, target, logits)
    tt = target == 1
    lo, hi = pp & ~excused, pp | excused
    cnt = lambda q: torch.stack([(q & tt).sum(1), q.sum(1), tt.sum(1)], -1)
    return cnt(lo), cnt(hi)


# ================================================================ rows of tests/test_gpu_loss3d_paths.py: geometry plus seed
PAIRS = [(1.0, 0.1), (0.37, 0.1), (-2.5, 0.25), (1.0, 0.0)]          # (upstream gradient g, w_l2)
PLANT = [0.0, -0.0, 1e-3, -1e-3, 8.0, -8.0, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0]
# the 24 logits around a seam, groups s - 3 .. s + 2 (s = the first float4 group behind the seam); every target of the groups s - 1 and s is 1 and
# their logits are saturated negatives that differ position by position: where a max-scaled bound is blind (tests/test_loss3d_check.py)
SEAM = PLANT[:4] + [8.0, -8.0, 20.0, 88.0] + [-20.0, -88.0, -100.0, -20.0] + [-100.0, -20.0, -88.0, -100.0] + [100.0, -8.0, 20.0, -1e-3] + [88.0, 8.0, -0.0, 1e-3]
_BODY = 4 * ((UN - 1) * T_CAP + 100) + 2          # 'partial body'


def OBJ(rid, n1, n2, seed, tmode, pairs, seam, phases, why):
    """tmode: share of ones in t | 'zeros' | 'perfect' (t = (u > 0)); seam: element index of the planted seam (None: the row has none);
    phases: {(launch, pair): (body, remainder, tail)} the row is in the table for -- launch 'joint' (the forward and the backward with both gradients:
    one grid, sized by the larger pair), 'du' / 'dv' (the backward with that gradient alone: sized by its own pair)"""
    return dict(id=rid, n1=n1, n2=n2, seed=seed, tmode=tmode, pairs=pairs, seam=seam, phases=phases, why=why)


OBJECTIVE_ROWS = [
    OBJ('tail1', 945, 1575, 101, 0.3, PAIRS, None, {('joint', 1): (False, 'partial', 1), ('joint', 2): (False, 'partial', 3), ('du', 1): (False, 'partial', 1)},
        'remainder once, tails of 1 and 3'),
    OBJ('one group', 4, 0, 102, 0.5, PAIRS, None, {('joint', 1): (False, 'partial', 0)}, 'Dice only; one thread of one block does the work'),
    OBJ('below a group', 3, 2, 103, 0.5, PAIRS, None, {('joint', 1): (False, 'zero', 3), ('joint', 2): (False, 'zero', 2)}, 'n / 4 = 0: tail only'),
    OBJ('whole grid', 4 * 2 * L3_THREADS + 2, 0, 104, 0.3, PAIRS, None, {('joint', 1): (False, 'all', 2)}, 'two full blocks: every thread takes the remainder once'),
    OBJ('all phases', 4 * (UN * T_CAP + T_CAP // 2 + 37) + 3, 4 * (UN * T_CAP + T_CAP // 2 + 37) + 1, 105, 0.05, PAIRS[:2], 4 * UN * T_CAP,
        {('joint', 1): (True, 'partial', 3), ('joint', 2): (True, 'partial', 1)}, 'cap binds; body once for every thread; remainder for T/2 + 37 threads; tail'),
    OBJ('partial body', _BODY, 0, 106, 'perfect', PAIRS[1:3], 4 * (UN - 1) * T_CAP, {('joint', 1): (True, 'partial', 2)},
        'cap binds; 100 threads take the body; the others the remainder U - 1 times'),
    OBJ('body exact', 4 * 2 * UN * T_CAP, 0, 107, 'zeros', PAIRS[:2], 4 * UN * T_CAP, {('joint', 1): (True, 'zero', 0)}, 'two body iterations, nothing after'),
    OBJ('big u small v', _BODY, 1575, 108, 0.3, PAIRS[1:3], 4 * (UN - 1) * T_CAP,
        {('joint', 1): (True, 'partial', 2), ('joint', 2): (False, 'partial', 3), ('dv', 2): (False, 'partial', 3)}, 'grid sized by pair 1; most threads idle on pair 2'),
    OBJ('small u big v', 945, _BODY, 109, 0.3, PAIRS[2:], 4 * (UN - 1) * T_CAP,
        {('joint', 1): (False, 'partial', 1), ('joint', 2): (True, 'partial', 2), ('du', 1): (False, 'partial', 1)}, 'the reverse; du alone runs on one block'),
]
OBJECTIVE = {r['id']: r for r in OBJECTIVE_ROWS}
# combinations of l3_stream's phases no row targets, and why
NOT_IN_TABLE = {
    'body and then the remainder for EVERY thread': 'needs U T + T <= n / 4 on a capped grid: 10.5 M floats for one more trip count of the loop that "all phases" enters '
                                                     'with half its threads and "partial body" with all but 100 of them, up to U - 1 times',
    'body with a tail of 0 behind a remainder': 'the tail test is one comparison on tid after both loops; "body exact" has tail 0, "all phases" tails 3 and 1, "partial body" 2',
}


def launch_threads(row, launch):
    n1, n2 = row['n1'], row['n2']
    return L3_THREADS * l3_blocks(n1 if launch != 'dv' else 0, n2 if launch != 'du' else 0)


@functools.lru_cache(maxsize=1)
def objective_case(rid):
    """-> dict(u, t (n1,), v, x (n2,) | None, shape1, shape2): the row's inputs, flat in memory order.  Logits N(0, 3) with PLANT at the head and in the
    last whole groups, SEAM around the row's seam, and the n % 4 tail at u = +8, t = 1, v = x + 4 (a dropped tail then moves A0, P2, T2 by about 1
    each and SE by 16 per element); v, x N(0, 1/4)"""
    row = OBJECTIVE[rid]
    n1, n2 = row['n1'], row['n2']
    g = torch.Generator().manual_seed(row['seed'])
    u = 3.0 * torch.randn(n1, generator=g)
    nv4 = 4 * (n1 // 4)
    if n1 >= 64:
        u[:12] = torch.tensor(PLANT)
        u[nv4 - 12:nv4] = torch.tensor(PLANT)
    if row['seam'] is not None and row['seam'] + 12 <= nv4:
        u[row['seam'] - 12:row['seam'] + 12] = torch.tensor(SEAM)
    u[nv4:] = 8.0
    if row['tmode'] == 'zeros':
        t = torch.zeros(n1)
    elif row['tmode'] == 'perfect':
        t = (u > 0).float()
    else:
        t = (torch.rand(n1, generator=g) < row['tmode']).float()
        if row['seam'] is not None and row['seam'] + 12 <= nv4:
            t[row['seam'] - 4:row['seam'] + 4] = 1.0
        t[nv4:] = 1.0
    v = x = None
    if n2:
        v, x = 0.25 * torch.randn(n2, generator=g), 0.25 * torch.randn(n2, generator=g)
        x[4 * (n2 // 4):] = 0.5
        v[4 * (n2 // 4):] = 4.5
    return dict(rid=rid, u=u, t=t, v=v, x=x, n1=n1, n2=n2, shape1=shape5(n1), shape2=shape5(n2))


# the layout rows: ONE flat buffer of the 'tail1' size per tensor under four stride sets of the logical shape (1, C, 5, 7, 9) -> (name, strides(C), shared)
LAYOUT_DHW = (5, 7, 9)


def layout_strides(C):
    D, H, W = LAYOUT_DHW
    return [
        ('dense NCDHW', (C * D * H * W, D * H * W, H * W, W, 1)),
        ('channels-last-3d', (C * D * H * W, 1, H * W * C, W * C, C)),
        ('storage order (D, B, W, C, H)', (W * C * H, H, W * C * H, 1, C * H)),          # strides of (B, C, D, H, W)
        ('B = 1, batch strides differ', (C * D * H * W, 1, H * W * C, W * C, C)),        # u as channels-last-3d; t: stride(0) replaced, see LAYOUT_BATCH_STRIDE_T
    ]


LAYOUT_BATCH_STRIDE_T = 7


# ---------------------------------------------------------------- seg_counts rows
def SEG(rid, B, C, P, vec, path, offset=0, blocks=None):
    """vec: the VEC instantiation is launched; offset: floats the base pointers sit behind a 16-byte boundary; blocks: (wanted, launched) along x"""
    return dict(id=rid, B=B, C=C, P=P, vec=vec, path=path, offset=offset, blocks=blocks)


SEG_ROWS = [
    SEG('vec, whole groups 2x3x64', 2, 3, 64, True, 'VEC, every group whole'),
    SEG('vec C1 2x1x1032', 2, 1, 1032, True, 'VEC, C = 1, two blocks'),
    SEG('vec, short last group 2x4x5', 2, 4, 5, True, 'VEC kernel, scalar fall-back for left < 4 C'),
    SEG('vec, short last group 1x2x6', 1, 2, 6, True, 'VEC kernel, scalar fall-back for left < 4 C'),
    SEG('scalar, ragged 2x3x315', 2, 3, 315, False, '(P C) % 4 != 0'),
    SEG('scalar, ragged 3x1x7', 3, 1, 7, False, '(P C) % 4 != 0'),
    SEG('scalar, ragged 2x2x7', 2, 2, 7, False, '(P C) % 4 != 0, C = 2'),
    SEG('scalar, by base 2x4x64', 2, 4, 64, False, 'non-VEC by alignment only', offset=1),
    SEG('sample starts 3x2x6', 3, 2, 6, True, 'P C = 12: every sample starts on a 16-byte boundary, last group short'),
    SEG('sample starts 3x4x3', 3, 4, 3, True, 'P C = 12, P < 4: the only group is short'),
    SEG('grid cap 64x3x33001', 64, 3, 33001, False, 'cap L3_MAX_BLOCKS / 64 below the blocks wanted: grid-stride', blocks=(33, 32)),
    SEG('cap floor %dx1x1101' % (L3_MAX_BLOCKS + 1), L3_MAX_BLOCKS + 1, 1, 1101, False, 'cap 1: one block strides over 276 groups', blocks=(2, 1)),
]
SEG_BY_ID = {r['id']: r for r in SEG_ROWS}


def seg_geometry(row):
    """the source's launch_seg_counts: (VEC, blocks wanted along x, blocks launched, groups per sample, groups that take the scalar fall-back in the VEC kernel)"""
    B, C, P = row['B'], row['C'], row['P']
    ngrp = (P + 3) >> 2
    want = -(-ngrp // L3_THREADS)
    cap = max(L3_MAX_BLOCKS // B, 1)
    vec = (P * C) % 4 == 0 and row['offset'] % 4 == 0
    return dict(vec=vec, want=want, launched=min(want, cap), ngrp=ngrp, short=int(vec and P % 4 != 0))


@functools.lru_cache(maxsize=2)
def seg_case(rid):
    """-> dict(logits, probs, target (B, P, C) fp32, planted: counts of the planted values).  Logits N(0, 3); eight exact zeros (the probabilities: exact
    0.5) on voxels labelled 1; four targets of 0.99999994 and four of 2.0 on voxels predicted beyond doubt (u = 3); in rows of 100,000 voxels and
    more, sixteen logits within the excused band (the probabilities: the fp32 neighbours of 0.5)"""
    row = SEG_BY_ID[rid]
    B, C, P = row['B'], row['C'], row['P']
    g = torch.Generator().manual_seed(1000 + B + 7 * C + P)
    n = B * P * C
    u = 3.0 * torch.randn(n, generator=g)
    t = (torch.rand(n, generator=g) > 0.6).float()
    perm = torch.randperm(n, generator=g)
    assert n >= 12
    zeros, near1, twos = perm[:8], perm[n - 8:n - 4], perm[n - 4:]          # (a row of fewer than 16 elements: some zeros carry a 0.99999994)
    u[near1] = 3.0; u[twos] = 3.0
    u[zeros] = torch.tensor([0.0, -0.0] * 4)
    t[zeros] = 1.0; t[near1] = 0.99999994; t[twos] = 2.0
    band = perm[16:32] if n >= 100000 else perm[:0]
    u[band] = torch.tensor([1e-7, -1e-7, 5e-7, -5e-7, 9e-7, -9e-7, 3e-8, -3e-8] * 2)[:len(band)]
    p = torch.sigmoid(u)
    p[zeros] = 0.5
    if len(band):
        p[band] = torch.tensor([0.5 + 2.0 ** -24, 0.5 - 2.0 ** -25] * 8)
    shape = (B, P, C)
    return dict(logits=u.reshape(shape), probs=p.reshape(shape), target=t.reshape(shape), zeros=zeros, near1=near1, twos=twos, band=band)


# kappa per (operation, output) of the rows above: 4 x the worst yardstick ratio SEEN over the operation's rows (the plain torch evaluation on the CPU
# against the float64 reference; in the comment), rounded up, at least 1 -- NOT taken from the kernels under test.  tests/test_loss3d_check.py holds the
# table to the rows' yardsticks without a GPU; profiles/loss3d_path_margins.txt lists the yardstick beside the kernels' ratio per row.  fp32 torch
# rounds a little differently from CPU to CPU: the table is set from the CPU the suite was written on; the host of the MI355X measured du at 3.36 on
# the same rows (the yardstick column of profiles/loss3d_path_margins.txt), inside the entry and inside the two-sided hold of tests/test_loss3d_check.py.
# Summation orders of the kernels that differ from the yardstick's (all inside their entries):
#   sums: thread (fp64 fma chain over its grid-stride elements) -> wave shuffles -> four waves -> 2048 partial rows -> one workgroup, all in fp64: what is
#     left beside the rounding of p is 1e-16 relative, nothing a kappa in units of 2^-24 sees.  The yardstick sums in float64 too; both carry the fp32
#     sigmoid's error only, and the kernel's expf + IEEE division need not round p as torch's vectorised sigmoid does.
KAPPA = {
    #                     kappa     yardstick
    ('fwd', 'sums'):          3,    #    0.56
    ('fwd', 'dice'):          2,    #    0.45
    ('fwd', 'l2'):            2,    #    0.35
    ('fwd', 'obj'):           3,    #    0.69
    ('bwd', 'du'):           13,    #    3.16
    ('bwd', 'dv'):           11,    #    2.69
}
