"""The element-wise float64 bound of tests/conv_check.py against the max-scaled close() of tests/test_gpu_ops.py, on the CPU: faults planted into a
float64 convolution result that a wrong tail mask or a mis-offset epilogue would produce are caught by the new bound and passed by close() at the
rtol the suite uses for that dtype; clean fp32- and bf16-rounded results pass the new bound (it is not vacuous); a coarse fault fails both.
The 3-D references (fwd_ref3d, dgrad_ref3d, wgrad_ref3d) get the same treatment, plus a tap lost on one depth face of the volume.
The bf16 weight-gradient rows of tests/test_gpu_conv_paths.py are held to the planner's replay (tests/bwgrad_plan.py) and to the plain fp32
evaluation their kappa derives from, with the faults of that family planted into it."""
import pytest
import torch

import bwgrad_plan as P
import conv_check as CC
import test_gpu_conv_paths as T
from test_gpu_ops import BWGRAD_PAIR, close

KAPPA = 64          # a stand-in for the per-kernel constants of tests/conv_check.py (1 .. 25 outside the F(4x4) Winograd forms and c4_mixed)
RTOL = {'fp32': 1e-4, 'bf16': 1.5e-2}          # what tests/test_gpu_ops.py uses today for these results


def layer(Ci, Co=40, N=2, H=9, W=11, seed=0, bf16=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Ci, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Co, Ci, 3, 3, generator=g, dtype=torch.float64) * (9 * Ci) ** -0.5
    b = torch.randn(Co, generator=g, dtype=torch.float64) * 0.1
    if bf16:
        x, w = CC.bf16_round(x), CC.bf16_round(w)
    ref, A = CC.fwd_ref(x, w, b, 1, 1)
    return x, w, b, ref, A


def stored(ref, dtype):
    """the float64 result as a kernel would store it"""
    return CC.bf16_round(ref) if dtype == 'bf16' else ref.float().double()


def new_check_catches(got, ref, A, dtype):
    with pytest.raises(AssertionError):
        CC.check(got, ref, A, KAPPA, u_out=CC.U_BF16 if dtype == 'bf16' else 0.0, what='planted fault')


@pytest.mark.parametrize('dtype,Ci', [('fp32', 16), ('fp32', 512), ('bf16', 512)])
def test_clean_results_pass_the_bound(dtype, Ci):
    x, w, b, ref, A = layer(Ci, bf16=dtype == 'bf16')
    r = CC.check(stored(ref, dtype), ref, A, KAPPA, u_out=CC.U_BF16 if dtype == 'bf16' else 0.0, what='clean')
    assert r <= 1.0, r                   # storing the exact result costs at most one unit of u A (fp32) / nothing beyond u_out |ref| (bf16)
    ref_l, _ = CC.fwd_ref(x, w, b, 1, 1, lrelu=True)
    CC.check(stored(ref_l, dtype), ref_l, A, KAPPA, u_out=CC.U_BF16 if dtype == 'bf16' else 0.0, what='clean + LeakyReLU')


@pytest.mark.parametrize('dtype,Ci,scale', [('bf16', 512, 2e-2), ('fp32', 16, 1e-4), ('fp32', 512, 1e-4)])
def test_cout_tail_fault_caught_by_the_bound_missed_by_close(dtype, Ci, scale):
    """the last 8 couts of a Co = 40 result scaled by 1 + scale: a wrong tail mask / a mis-offset epilogue"""
    _, _, _, ref, A = layer(Ci, bf16=dtype == 'bf16')
    got = stored(ref, dtype).clone()
    got[:, -8:] *= 1 + scale
    close(got, ref, rtol=RTOL[dtype], what='close() passes the fault')
    new_check_catches(got, ref, A, dtype)


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_dropped_tap_caught_by_both(dtype):
    """the centre tap of the last 8-channel chunk dropped on the top border row (a tap that reads real data, not the zero padding)"""
    Ci = 512
    x, w, b, ref, A = layer(Ci, bf16=dtype == 'bf16', H=6, W=6, Co=40)
    lost = torch.einsum('nch,oc->noh', x[:, -8:, 0, :], w[:, -8:, 1, 1])            # (N, Co, W): what the centre tap adds to row 0
    got = stored(ref, dtype).clone()
    got[:, :, 0, :] -= lost
    new_check_catches(got, ref, A, dtype)
    with pytest.raises(AssertionError):
        close(got, ref, rtol=RTOL[dtype], what='coarse fault')


def test_nan_and_misplaced_elements_fail():
    _, _, _, ref, A = layer(16)
    got = ref.clone(); got[0, 3, 4, 5] = float('nan')
    with pytest.raises(AssertionError):
        CC.check(got, ref, A, KAPPA)
    assert CC.ratio(got, ref, A) == float('inf')
    got = ref.clone(); got[1, 0] = ref[1, 1]
    with pytest.raises(AssertionError):
        CC.check(got, ref, A, KAPPA)


def test_reference_gradients_match_autograd():
    """the data- and weight-gradient references are the adjoints of the forward one"""
    g = torch.Generator().manual_seed(3)
    for (Ci, Co, k, s, p, H, W) in [(5, 6, 3, 1, 1, 9, 11), (7, 16, 4, 2, 1, 10, 12), (4, 6, 3, 2, 1, 11, 13)]:
        x = torch.randn(2, Ci, H, W, generator=g, dtype=torch.float64, requires_grad=True)
        w = torch.randn(Co, Ci, k, k, generator=g, dtype=torch.float64, requires_grad=True)
        b = torch.randn(Co, generator=g, dtype=torch.float64, requires_grad=True)
        y = torch.nn.functional.conv2d(x, w, b, s, p)
        dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        y.backward(dy)
        dx, Adx = CC.dgrad_ref(dy, w.detach(), (H, W), s, p)
        dw, Adw, db, Adb = CC.wgrad_ref(x.detach(), dy, k, k, s, p)
        assert torch.allclose(dx, x.grad) and torch.allclose(dw, w.grad) and torch.allclose(db, b.grad)
        assert (Adx >= dx.abs() - 1e-12).all() and (Adw >= dw.abs() - 1e-12).all() and (Adb >= db.abs()).all()


# ---------------------------------------------------------------- 3-D (tests/test_gpu_conv3d_paths.py)
def layer3d(Ci, Co=20, N=2, D=5, H=6, W=7, seed=0, residual=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Ci, D, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Co, Ci, 3, 3, 3, generator=g, dtype=torch.float64) * (27 * Ci) ** -0.5
    b = torch.randn(Co, generator=g, dtype=torch.float64) * 0.1
    res = torch.randn(N, Co, D, H, W, generator=g, dtype=torch.float64) if residual else None
    ref, A = CC.fwd_ref3d(x, w, b, 1, 1, res)
    return x, w, b, ref, A


@pytest.mark.parametrize('Ci,residual', [(16, False), (128, True)])
def test_clean_3d_results_pass_the_bound(Ci, residual):
    _, _, _, ref, A = layer3d(Ci, residual=residual)
    r = CC.check(stored(ref, 'fp32'), ref, A, KAPPA, what='clean 3-D')
    assert r <= 1.0, r


@pytest.mark.parametrize('Ci,residual', [(16, False), (128, True)])
def test_3d_cout_tail_fault_caught_by_the_bound_missed_by_close(Ci, residual):
    """the last 4 couts of a Co = 20 3-D result scaled by 1 + 1e-4: passes the 1e-3 max-scaled check tests/test_gpu_3d.py uses"""
    _, _, _, ref, A = layer3d(Ci, residual=residual)
    got = stored(ref, 'fp32').clone()
    got[:, -4:] *= 1 + 1e-4
    close(got, ref, rtol=1e-3, what='close() passes the fault')
    new_check_catches(got, ref, A, 'fp32')


@pytest.mark.parametrize('face', ['first', 'last'])
def test_3d_tap_dropped_on_a_depth_face_fails_the_bound(face):
    """one depth tap of the last 8 input channels lost on the first (or last) D plane only -- the tap that reads the real neighbouring plane,
    not the zero padding: a wrong depth-halo mask in a box at the volume boundary"""
    Ci = 64
    x, w, b, ref, A = layer3d(Ci, D=6, H=5, W=6)
    d, r, src = (0, 2, 1) if face == 'first' else (-1, 0, -2)        # out plane, depth tap, the input plane that tap reads
    lost = torch.einsum('nchw,oc->nohw', x[:, -8:, src], w[:, -8:, r, 1, 1])
    got = stored(ref, 'fp32').clone()
    got[:, :, d, 1:, :] -= lost[:, :, 1:, :]          # (every row but the first: the fault is confined to part of one face)
    new_check_catches(got, ref, A, 'fp32')


def test_3d_reference_gradients_match_autograd():
    """the 3-D data- and weight-gradient references are the adjoints of the forward one; the fused residual enters ref and A"""
    g = torch.Generator().manual_seed(5)
    for (Ci, Co, s, D, H, W) in [(5, 6, 1, 4, 5, 6), (4, 10, 2, 5, 7, 6), (3, 8, 2, 1, 3, 4)]:
        x = torch.randn(2, Ci, D, H, W, generator=g, dtype=torch.float64, requires_grad=True)
        w = torch.randn(Co, Ci, 3, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
        b = torch.randn(Co, generator=g, dtype=torch.float64, requires_grad=True)
        y = torch.nn.functional.conv3d(x, w, b, s, 1)
        res = torch.randn(y.shape, generator=g, dtype=torch.float64)
        ref, A = CC.fwd_ref3d(x.detach(), w.detach(), b.detach(), s, 1, res)
        assert torch.allclose(ref, y.detach() + res) and (A >= ref.abs() - 1e-12).all()
        dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        y.backward(dy)
        dx, Adx = CC.dgrad_ref3d(dy, w.detach(), (D, H, W), s, 1)
        dw, Adw, db, Adb = CC.wgrad_ref3d(x.detach(), dy, 3, s, 1)
        assert torch.allclose(dx, x.grad) and torch.allclose(dw, w.grad) and torch.allclose(db, b.grad)
        assert (Adx >= dx.abs() - 1e-12).all() and (Adw >= dw.abs() - 1e-12).all() and (Adb >= db.abs()).all()


# ---------------------------------------------------------------- the bf16 weight-gradient rows (tests/test_gpu_conv_paths.py BW_ROWS)
# Their kappa does not come from the kernels: it is 4x the worst ratio of the rows' own sums evaluated in plain fp32 by torch on the CPU
# (CC.wgrad_fp32) against the rows' float64 reference.  Here, without a GPU: the planner's replay says each row reaches the kernel and
# instantiation its id names on 256 CUs; the yardstick passes the bound at the committed kappa and the kappa is no looser than four times its rule
# on the CPU this runs on; and five faults that the family's kernels could plausibly commit, planted into the yardstick, fail the bound.
BW_FAMILIES = ('bwgrad', 'bwgrad2', 'bwgrad3', 'bwgrad_s2')


@pytest.fixture(autouse=True)
def _cpu_threads():
    """the references and the yardstick on at most 16 CPU threads"""
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    yield
    torch.set_num_threads(n)


def bw_row(rid):
    return next(p.values[0] for p in T.BW_ROWS if p.id == rid)


def bw_plan(row):
    N, Ci, Co, H, W, k, st, pad = row['geom']
    return P.plan(N, Ci, Co, H, W, k, st, pad, dtype=row['dtype'], opts=row['opts'], ld_ok=row['in_pad'] is None)


def test_bwgrad_rows_reach_every_instantiation_on_256_cus():
    """the replayed planner gives every row the kernel it expects and the instantiation in its id; together the rows cover all 24 instantiations
    of the four kernels and the three phases of the reduce kernel's slab loop; the fallback rows are declined"""
    seen, phases = set(), set()
    for p in T.BW_ROWS:
        row, pl = p.values[0], bw_plan(p.values[0])
        assert pl is not None and row['expect'] == (pl['kernel'],) and p.id.startswith(pl['kernel'] + pl['inst']), (p.id, pl)
        assert row['op'] == 'wgrad' and row['launches'] == 2
        seen.add((pl['kernel'], pl['inst']))
        phases.add(P.reduce_phase(pl['splits']))
        if row['twin']:
            twin = P.plan(*row['geom'], dtype=row['dtype'], opts={**row['opts'], **row['twin'][0]})
            assert twin['kernel'] == row['twin'][1] != pl['kernel'] and twin['splits'] == pl['splits']
    ab = [(a, b) for a in (1, 2) for b in (1, 2)]
    want = ({('bwgrad', f'<{a},{b},{ts}>') for a, b in ab for ts in ('__bf16', 'float')} | {('bwgrad', f'<1,{b},__bf16,HALF>') for b in (1, 2)}
            | {(k, f'<{a},{b}>') for k in ('bwgrad2', 'bwgrad3') for a, b in ab}
            | {('bwgrad_s2', f'<{a},{b},false>') for a, b in ab} | {('bwgrad_s2', f'<1,{b},HALF>') for b in (1, 2)})
    assert seen == want and len(want) == 24, (want - seen, seen - want)
    assert {'one slab per wave at most', 'tail only, several slabs per wave', 'unrolled body + tail'} <= phases, phases
    sinks = [p.values[0]['sink'] for p in T.BW_ROWS]
    assert all(a != b for a, b in zip(sinks, sinks[1:]))
    nat = bw_plan(bw_row('bwgrad2<1,1> natural window'))
    assert not bw_row('bwgrad2<1,1> natural window')['opts'] and 2 * nat['splits'] <= nat['tiles'] < 3 * nat['splits']
    fell = [p for p in T.ROWS if p.values[0]['fallback']]
    assert len(fell) == 3 and all(bw_plan(p.values[0]) is None for p in fell)
    one = next(p.values[0] for p in fell if p.values[0]['in_pad'])          # declined for its pixel stride alone
    assert (one['geom'][1] + sum(one['in_pad'])) % 8 != 0 and P.plan(*one['geom'], opts=one['opts'])['kernel'] == 'bwgrad'
    for case, (k2, k3) in BWGRAD_PAIR.items():                             # tests/test_gpu_ops.py test_bf16_weight_gradient_lds_dma_bit_identical
        assert (P.plan(*case, opts={'debug_mode': 3010})['kernel'], P.plan(*case)['kernel']) == (k2, k3), case


def test_bwgrad_kappa_is_four_times_the_fp32_yardstick():
    worst = {f: 0.0 for f in BW_FAMILIES}
    for p in T.BW_ROWS:
        row = p.values[0]
        y = T.wgrad_yardstick(row)
        kappa = CC.KAPPA[(row['kname'], 'wgrad')]
        assert max(y.values()) <= kappa, (p.id, y, kappa)                  # the unfaulted yardstick passes every row
        worst[row['kname']] = max(worst[row['kname']], *y.values())
    for f in BW_FAMILIES:
        kappa = CC.KAPPA[(f, 'wgrad')]
        # the rule is max(1, 4 worst).  The worst moves with the CPU's summation order -- two hosts gave 4.29 and 3.31 for 'bwgrad3', 2.43 and
        # 1.34 for 'bwgrad', on single rows 4.29 and 2.19 -- so the constant is held to four times the rule, not to the rule itself
        assert kappa >= 1 and kappa <= max(1.0, 16 * worst[f]), (f, kappa, worst[f])


def _stale_mask(row):
    """for a workgroup that walks the tiles t, t + slabs, t + 2 slabs, ... through a ring of three stages: (n, rows, cols) of a ragged tile's masked
    in-tile positions and the image n2 and offsets of the tile two steps earlier, whose values a missing zero fill would leave there"""
    N, Ci, Co, H, W = row['geom'][:5]
    pl = bw_plan(row)
    assert pl['NB'] == 1
    TH, TW, tA, tB = pl['TH'], pl['TW'], P.cdiv(H, pl['TH']), P.cdiv(W, pl['TW'])
    for t in range(pl['tiles'] - 1, 2 * pl['splits'] - 1, -1):
        tb, ta, n = t % tB, (t // tB) % tA, t // (tB * tA)
        t2 = t - 2 * pl['splits']
        tb2, ta2, n2 = t2 % tB, (t2 // tB) % tA, t2 // (tB * tA)
        h_valid, w_valid = min(TH, H - ta * TH), min(TW, W - tb * TW)
        h2_valid, w2_valid = min(TH, H - ta2 * TH), min(TW, W - tb2 * TW)
        if h_valid < TH and h2_valid == TH and w2_valid == TW:      # rows h_valid .. TH - 1 of the tile are masked; the earlier tile was full
            return n2, slice(ta2 * TH + h_valid, ta2 * TH + TH), slice(tb2 * TW, tb2 * TW + TW)
    raise AssertionError('no ragged tile behind a full one')


FAULTS = ['position dropped', 'stale ring stage', 'taps swapped', 'HALF rows folded', 'bias from rounded dy']


@pytest.mark.parametrize('fault', FAULTS)
def test_planted_bwgrad_fault_fails_the_rows_bound(fault):
    rid = {'position dropped': 'bwgrad3<1,1> ragged in H and W', 'stale ring stage': 'bwgrad3<1,1> ragged in H and W',
           'taps swapped': 'bwgrad_s2<1,1,false> 3x3', 'HALF rows folded': 'bwgrad<1,1,__bf16,HALF>', 'bias from rounded dy': 'bwgrad<1,2,float>'}[fault]
    row = bw_row(rid)
    N, Ci, Co, H, W, k, st, pad = row['geom']
    kappa = CC.KAPPA[(row['kname'], 'wgrad')]
    x, dy, ref_w, A_w, ref_b, A_b = T.wgrad_operands(row['geom'], row['dtype'])
    dw, db = CC.wgrad_fp32(x, dy, k, st, pad, rounded_bias=row['dtype'] != 'bf16m')
    CC.check(dw, ref_w, A_w, kappa, what='yardstick dw')
    CC.check(db, ref_b, A_b, kappa, what='yardstick db')
    xb, yb = x.to(torch.bfloat16).float(), dy.to(torch.bfloat16).float()
    shape = (Co, Ci, k, k)
    bad_w, bad_b = dw.clone(), db.clone()
    if fault == 'position dropped':                 # the one valid position of the corner tile (last row, last column) of image 2
        one = torch.zeros_like(yb[2:3]); one[0, :, H - 1, W - 1] = yb[2, :, H - 1, W - 1]
        bad_w -= torch.nn.grad.conv2d_weight(xb[2:3], shape, one, st, pad)
    elif fault == 'stale ring stage':               # the masked rows of a ragged tile still hold the tile the stage was filled with two steps earlier
        n2, rows, cols = _stale_mask(row)
        old = torch.zeros_like(yb[n2:n2 + 1]); old[0, :, rows, cols] = yb[n2, :, rows, cols]
        bad_w += torch.nn.grad.conv2d_weight(xb[n2:n2 + 1], shape, old, st, pad)
    elif fault == 'taps swapped':                   # two taps of the odd-odd parity class land on each other's place in the tap map
        bad_w[:, :, 0, 0], bad_w[:, :, 0, 2] = dw[:, :, 0, 2], dw[:, :, 0, 0]
    elif fault == 'HALF rows folded':               # the 16 channels that follow a 16-channel slice in memory, summed into its rows
        after = torch.randn(N, 16, H, W, generator=torch.Generator().manual_seed(12)).to(torch.bfloat16).float()
        bad_w += torch.nn.grad.conv2d_weight(after, shape, yb, st, pad)
    else:                                           # fp32 views: the kernel sums the bias before it rounds dy for the MFMA
        assert row['dtype'] == 'bf16m'
        bad_b = yb.sum((0, 2, 3))
    with pytest.raises(AssertionError):
        if fault == 'bias from rounded dy':
            CC.check(bad_b, ref_b, A_b, kappa, what=fault)
        else:
            CC.check(bad_w, ref_w, A_w, kappa, what=fault)
