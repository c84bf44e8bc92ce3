"""tests/loss3d_check.py on the CPU: the plain torch evaluation of every row of tests/test_gpu_loss3d_paths.py (its TorchImpl: the yardstick) passes its own
bound; loss3d_check.KAPPA is what the yardsticks say (4 x the worst ratio of the operation's rows, at least 1); the rows reach the phases of l3_stream
and the seg_counts instantiations they name; and faults planted into a correct fp32 result -- a dropped n % 4 tail, a dropped remainder range, a float4
group stored one group off, an ignored upstream gradient, a term dropped on the labelled voxels, a fast sigmoid, the wrong element count -- are
rejected by check() at the row's own size, from the float64 and fp32 CPU evaluations alone.  One of them PASSES the global bound of
tests/test_gpu_loss3d.py (max |got - ref64| <= max(2 max |torch32 - ref64|, 4 u max |ref64|)), written out below: that is why this suite exists."""
import math

import pytest
import torch

import loss3d_check as LC
import test_gpu_loss3d_paths as G

YARD = G.TorchImpl()
T, UN = LC.T_CAP, LC.UN
G_UP, W_L2 = 0.37, 0.1
G32 = LC.f32(G_UP)          # what the fp32 evaluation multiplies by


@pytest.fixture(autouse=True, scope='module')
def _cpu_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    yield
    torch.set_num_threads(n)


def rejected(got, ref, A, key):
    with pytest.raises(AssertionError):
        LC.check(got, ref, A, LC.KAPPA[key], what='planted fault')


# ---------------------------------------------------------------- every row in plain torch
@pytest.fixture(scope='module')
def yardsticks():
    """{row id: [(output, key, ratio)]} of every row of the GPU suite under TorchImpl (the seg_counts rows assert their own interval)"""
    return {p.id: G.run_row(p.values[0], p.values[1], YARD, p.id, False) for p in G.ALL_ROWS}


def test_fp32_torch_passes_every_bound(yardsticks):
    bad = [(rid, name, key, r) for rid, items in yardsticks.items() for name, key, r in items if not r <= LC.KAPPA[key]]
    assert not bad, bad


def test_kappa_is_four_times_the_worst_yardstick(yardsticks):
    worst = {}
    for items in yardsticks.values():
        for _, key, r in items:
            worst[key] = max(worst.get(key, 0.0), r)
    assert set(worst) == set(LC.KAPPA), set(worst) ^ set(LC.KAPPA)
    for key, w in worst.items():
        assert w <= LC.KAPPA[key] <= max(1, math.ceil(4.0 * w)) + 1, (key, w, LC.KAPPA[key])


def test_rows_reach_the_paths_they_name():
    G.test_table_covers_every_path()


# ---------------------------------------------------------------- planted faults, at the size of 'all phases'
class Case:
    pass


@pytest.fixture(scope='module')
def big():
    """'all phases' (9.4 M floats per tensor) under the yardstick at g = 0.37, w_l2 = 0.1, with its float64 references"""
    k = Case()
    k.row = LC.OBJECTIVE['all phases']
    k.c = c = LC.objective_case('all phases')
    k.o = LC.objective_t(c['u'], c['t'], c['v'], c['x'], W_L2, G_UP)
    k.sums = LC.sums_t(c['u'], c['t'], c['v'], c['x'])
    k.sref = LC.sums_ref(c['u'], c['t'], c['v'], c['x'])
    k.duref = LC.du_ref(c['u'], c['t'], k.o['stored'], G32)
    k.end64 = LC.du_ref(c['u'], c['t'], k.sref[0], G32)[0]          # float64 from the inputs alone, as tests/test_gpu_loss3d.py forms its reference
    k.nv4, k.seam = 4 * (c['n1'] // 4), k.row['seam']
    assert k.seam == 4 * UN * T and k.nv4 > k.seam and c['n1'] - k.nv4 == 3 and c['n2'] % 4 == 1
    LC.check(k.sums, *k.sref, LC.KAPPA[('fwd', 'sums')], what='clean sums')
    LC.check(k.o['du'], *k.duref, LC.KAPPA[('bwd', 'du')], what='clean du')
    return k


def old_global_bound_accepts(got, torch32, ref64):
    """tests/test_gpu_loss3d.py: max |got - ref64| <= max(2 max |torch32 - ref64|, FLOOR_ULPS 2^-24 max |ref64|), FLOOR_ULPS = 4"""
    e_torch, e_got = float((torch32.double() - ref64).abs().max()), float((got.double() - ref64).abs().max())
    return e_got <= max(2 * e_torch, 4 * 2.0 ** -24 * float(ref64.abs().max()))


def part_sums(c, a1, b1, a2, b2):
    """the yardstick's sums over u, t [a1, b1) and v, x [a2, b2)"""
    return LC.sums_t(c['u'][a1:b1], c['t'][a1:b1], c['v'][a2:b2], c['x'][a2:b2])


def test_fault_sums_without_the_tail(big):
    """a condition on the inputs, from the references alone: the three tail elements of (u, t) and the one of (v, x) move EVERY sum past its bound, by
    at least 4 x (they sit at u = +8, t = 1, v - x = 4: about 1, 1, 1 and 16 per element, in sums of 2e5 to 4e6)"""
    c = big.c
    nv2 = 4 * (c['n2'] // 4)
    tail = part_sums(c, big.nv4, c['n1'], nv2, c['n2'])
    assert tail[0] > 2.9 and tail[1] > 2.9 and tail[2] == 3.0 and tail[3] == 16.0
    short = big.sums - tail
    excess = (short - big.sref[0]).abs() / (LC.KAPPA[('fwd', 'sums')] * LC.U * big.sref[1])
    print('\n[loss3d check] dropped tail: |error| / bound per sum', [round(float(e), 1) for e in excess])
    assert float(excess.min()) >= 4.0, excess
    rejected(short, *big.sref, ('fwd', 'sums'))


def test_fault_sums_without_the_remainder(big):
    """[4 U T, 4 (n / 4)): what the remainder loop adds behind the unrolled body"""
    c = big.c
    short = big.sums - part_sums(c, big.seam, big.nv4, big.seam, 4 * (c['n2'] // 4))
    rejected(short, *big.sref, ('fwd', 'sums'))
    assert LC.ratio(short, *big.sref) > 1e5


def planted(big, lo, hi, values):
    du = big.o['du'].clone()
    du[lo:hi] = values
    return du


def test_fault_du_without_the_tail(big):
    du = planted(big, big.nv4, big.c['n1'], 0.0)
    rejected(du, *big.duref, ('bwd', 'du'))
    assert not old_global_bound_accepts(du, big.o['du'], big.end64)          # at u = +8 the old bound sees it too


def test_fault_du_without_the_remainder(big):
    rejected(planted(big, big.seam, big.nv4, 0.0), *big.duref, ('bwd', 'du'))


def test_fault_du_group_one_off_passes_the_global_bound(big):
    """the last float4 group of the unrolled body stored from its neighbour behind the seam.  The row plants saturated negative logits with t = 1 there:
    du = g c1 p there, 1e-9 of the largest gradient and below -- under any bound scaled by the maximum, and 1e7 u A"""
    s = big.seam
    assert bool((big.c['t'][s - 4:s + 4] == 1).all()) and float(big.c['u'][s - 4:s + 4].max()) <= -20
    du = planted(big, s - 4, s, big.o['du'][s:s + 4])
    assert not torch.equal(du, big.o['du'])
    assert old_global_bound_accepts(du, big.o['du'], big.end64)
    rejected(du, *big.duref, ('bwd', 'du'))
    assert LC.ratio(du, *big.duref) > 1e5


def test_fault_du_ignores_the_upstream_gradient(big):
    du = (big.o['du'].double() / G_UP).float()          # g = 1
    rejected(du, *big.duref, ('bwd', 'du'))


def fp32_du(big, p, mask, c1_on=True):
    """g (c1 t + c2 p) p (1 - p) on the masked voxels from the p handed in, rounded to fp32; the yardstick's du elsewhere"""
    a0, den, _ = LC._coef(big.o['stored'])
    c1, c2 = (-2.0 / den if c1_on else 0.0), 4.0 * a0 / (den * den)
    pd, td = p.double(), big.c['t'].double()
    return torch.where(mask, (G32 * (c1 * td + c2 * pd) * pd * (1 - pd)).float(), big.o['du'])


def test_fault_du_drops_c1_on_the_labelled_voxels(big):
    du = fp32_du(big, torch.sigmoid(big.c['u']), big.c['t'] == 1, c1_on=False)
    rejected(du, *big.duref, ('bwd', 'du'))


def test_fault_du_fast_sigmoid(big):
    """a sigmoid that is 1e-4 relative off beyond |u| = 8"""
    u = big.c['u']
    wide = u.abs() > 8
    assert int(wide.sum()) > 1000
    du = fp32_du(big, torch.sigmoid(u) * (1 + 1e-4), wide)
    rejected(du, *big.duref, ('bwd', 'du'))
    neg = wide & (u < 0)                               # ... and on the negative side alone, where p' (1 - p') moves by 1e-4 of itself
    rejected(fp32_du(big, torch.sigmoid(u) * (1 + 1e-4), neg), *big.duref, ('bwd', 'du'))


def test_fault_dv_divides_by_the_other_count():
    """n1 in place of n2, at 'tail1' (945 and 1575 floats)"""
    c = LC.objective_case('tail1')
    o = LC.objective_t(c['u'], c['t'], c['v'], c['x'], W_L2, G_UP)
    ref = LC.dv_ref(c['v'], c['x'], G32, W_L2)
    LC.check(o['dv'], *ref, LC.KAPPA[('bwd', 'dv')], what='clean dv')
    rejected((o['dv'].double() * c['n2'] / c['n1']).float(), *ref, ('bwd', 'dv'))


def test_nan_fails():
    c = LC.objective_case('tail1')
    ref = LC.dv_ref(c['v'], c['x'], G32, W_L2)
    got = ref[0].float()
    got[3] = float('nan')
    rejected(got, *ref, ('bwd', 'dv'))


# ---------------------------------------------------------------- seg_counts: conditions on the inputs, and the strictness of both comparisons
@pytest.mark.parametrize('rid', [r['id'] for r in LC.SEG_ROWS])
def test_seg_rows_plant_what_decides_the_comparisons(rid):
    c = LC.seg_case(rid)
    flat = lambda t: t.reshape(-1)
    for logits in (True, False):
        pred = c['logits'] if logits else c['probs']
        counts, excused = LC.seg_counts_ref(pred, c['target'], logits)
        lo, hi = LC.seg_counts_bounds(pred, c['target'], logits)
        assert bool((lo <= counts).all()) and bool((counts <= hi).all())
        assert float(excused.double().mean()) <= 1e-3 and int(excused.sum()) >= len(c['band'])          # (a large row draws a few more by itself)
        centre = 0.0 if logits else 0.5
        at = flat(pred) == centre
        assert int(at.sum()) >= 8 and bool((flat(pred)[c['zeros']] == centre).all()) and not bool(flat(excused)[at].any())
        # the float64 reference counts them as not predicted: counting them as predicted (>= in place of >) leaves the interval
        pp = (torch.sigmoid(pred.double()) if logits else pred.double()) >= 0.5
        tt = c['target'] == 1
        loose = torch.stack([(pp & tt).sum(1), pp.sum(1), tt.sum(1)], -1)
        assert bool((loose[..., 1] > hi[..., 1]).any())
        if not bool((flat(c['target'])[c['zeros']] != 1).all()):
            assert bool((loose[..., 0] > hi[..., 0]).any())
    special = (flat(c['target']) == 0.99999994) | (flat(c['target']) == 2.0)
    assert int(special.sum()) >= 8 and int((flat(c['target']) == 0.99999994).sum()) >= 4 and int((flat(c['target']) == 2.0).sum()) >= 4
    assert torch.tensor(0.99999994).item() < 1.0          # 1 - 2^-24 is an fp32 value of its own
    counts, _ = LC.seg_counts_ref(c['logits'], c['target'], True)
    near = torch.stack([((c['target'] - 1).abs() < 1e-6).sum(1), (c['target'] >= 1).sum(1)], -1)          # t within a rounding of 1; t >= 1
    assert bool((near[..., 0] > counts[..., 2]).any()) and bool((near[..., 1] > counts[..., 2]).any())
