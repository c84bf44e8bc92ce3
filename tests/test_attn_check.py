"""tests/attn_check.py on the CPU: the plain fp32 torch evaluation of every row of tests/test_gpu_attn_paths.py (its TorchImpl: the yardstick) passes its
own bound and every exact assertion; attn_check.KAPPA is what the yardsticks say (4 x the worst ratio of the operation's rows, at least 1); and faults
planted into a correct fp32 result -- what a mis-indexed channel, a dropped term, a skipped pixel chunk, a short batch loop, a wrong prior row or a
clamp one short would produce -- PASS the max-scaled comparisons of tests/test_gpu_output_decoders.py / test_gpu_latent_options.py at their own
tolerances and are rejected by check(), each demonstrated at its inputs."""
import math

import pytest
import torch

import attn_check as AT
import test_gpu_attn_paths as G

YARD = G.TorchImpl()


def rejected(got, ref, A, key):
    with pytest.raises(AssertionError):
        AT.check(got, ref, A, AT.KAPPA[key], what='planted fault')


def old_err(got, want):
    """tests/test_gpu_output_decoders.py _err: the largest error over the largest reference value"""
    want = want.double()
    return float((got.double() - want).abs().max()) / (float(want.abs().max()) + 1e-30)


def old_kl_close(got, want):
    """tests/test_gpu_latent_options.py close()"""
    return float((got.double() - want).abs().max()) <= 1e-5 * float(want.abs().max()) + 1e-7


# ---------------------------------------------------------------- every row in plain fp32 torch
@pytest.fixture(scope='module')
def yardsticks():
    """{row id: [(output, key, ratio)]} of every row of the GPU suite under TorchImpl (exact assertions included)"""
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    out = {p.id: G.run_row(p.values[0], p.values[1], YARD, p.id, False) for p in G.ALL_ROWS}
    torch.set_num_threads(n)
    return out


def test_fp32_torch_passes_every_bound(yardsticks):
    bad = [(rid, name, key, r) for rid, items in yardsticks.items() for name, key, r in items if not r <= AT.KAPPA[key]]
    assert not bad, bad


def test_kappa_is_four_times_the_worst_yardstick(yardsticks):
    worst = {}
    for items in yardsticks.values():
        for _, key, r in items:
            worst[key] = max(worst.get(key, 0.0), r)
    assert set(worst) == set(AT.KAPPA), set(worst) ^ set(AT.KAPPA)
    # the rule of tests/test_aux_check.py: 4 x the worst yardstick SEEN; fp32 torch rounds a little differently from CPU to CPU (FMA contraction, how many
    # threads a sum is split over), so the table is held to ceil(4 w) with 15 % of slack on w either way
    for key, w in worst.items():
        assert AT.KAPPA[key] >= 1 and 4.0 * w / 1.15 <= AT.KAPPA[key] <= max(1, math.ceil(4.0 * w * 1.15)), (key, w, AT.KAPPA[key])


def test_rows_state_their_geometry():
    """the chatt rows reach what the table says: more than one channel group in either form, a last group of 1 and of 4, a width that does not divide
    the block, ragged chunks, the clamp of P, and every row's own (form, CG, P, last) agrees with chatt_geom (row_chatt asserts it)"""
    geoms = [p.values[0]['geom'] for p in G.CHATT_ROWS] + [p.values[0]['dense'] for p in G.CHATT_ROWS]
    assert any(g['V'] == 4 and g['CG'] == 2 and g['last'] == 1 for g in geoms) and any(g['V'] == 1 and g['CG'] == 2 and g['last'] == 4 for g in geoms)
    assert any(G.OD_THREADS % g['last'] for g in geoms) and any(g['P'] == 3 for g in geoms) and any(g['P'] == 16 for g in geoms)
    g = G.chatt_geom(2, 200, 64, 4)
    assert (g['P'], g['chunk']) == (3, 67) and 200 % 67          # three chunks of 67, 67, 66
    assert G.chatt_geom(1025, 4, 4, 4)['P'] == 1 and 1024 // 1025 == 0
    rows = {p.id: p.values[0] for p in G.CHATT_ROWS}
    assert G.is_v1(64, rows['chatt 2x64x8x8 Hd16 offset 1 scalar by alignment']['lay']) and sum(rows['chatt 2x64x8x8 Hd16 offset 1 scalar by alignment']['lay']) % 4 == 0
    lay = rows['chatt 2x64x8x8 Hd16 ld C+2 scalar by stride']['lay']
    assert lay[0] == 0 and (64 + sum(lay)) % 4 and G.is_v1(64, lay)


# ---------------------------------------------------------------- channel attention
def chatt_fault_case(B=2, C=64, HW=200, Hd=16):
    """the row's inputs (channel 1 of x, s, dy scaled by 1e-6) with that channel's column of W_down as small: a channel that hardly feeds the squeeze"""
    c = dict(G.chatt_case(B, C, HW, Hd))
    c['wd'] = c['wd'].clone()
    c['wd'][:, 1] *= 1e-6
    f = AT.chatt_fwd_t(c['x'], c['s'], c['wd'], c['bd'], c['wu'], c['bu'])
    return c, f


def chatt_end_to_end(c):
    """float64 from the inputs alone, as the old tests form their reference"""
    x, s, wd, bd, wu, bu = (c[k].double() for k in ('x', 's', 'wd', 'bd', 'wu', 'bu'))
    a = torch.sigmoid(torch.relu(x.mean(1) @ wd.T + bd) @ wu.T + bu)
    return a, (1 + a)[:, None, :] * x + s


def test_fault_wrong_a_in_a_small_channel():
    c, f = chatt_fault_case()
    ref = AT.chatt_out_ref(c['x'], c['s'], f['a'])
    AT.check(f['out'], *ref, AT.KAPPA[('chatt', 'out')], what='clean')
    out = f['out'].clone()
    out[:, :, 1] = (1 + f['a'][:, None, 0]) * c['x'][:, :, 1] + c['s'][:, :, 1]          # channel 1 gated by its neighbour's a
    assert old_err(out, chatt_end_to_end(c)[1]) <= 2e-6 / 10                              # far inside the old tolerance
    rejected(out, *ref, ('chatt', 'out'))
    assert AT.ratio(out, *ref) > 1e5


def test_fault_dpool_dropped_from_dx_in_a_small_channel():
    c, f = chatt_fault_case()
    b = AT.chatt_bwd_t(c['dy'], c['x'], f['a'], f['hid'], f['pool'], c['wd'], c['wu'])
    ref = AT.chatt_bwd_ref(c['dy'], c['x'], f['a'], f['hid'], f['pool'], c['wd'], c['wu'])
    for n in b:
        AT.check(b[n], *ref[n], AT.KAPPA[('chatt', n)], what='clean ' + n)
    dx = b['dx'].clone()
    dx[:, :, 1] = (1 + f['a'][:, None, 1]) * c['dy'][:, :, 1]
    assert old_err(dx, ref['dx'][0]) <= 2e-6 / 10
    rejected(dx, *ref['dx'], ('chatt', 'dx'))


def test_fault_one_pixel_chunk_skipped_in_pool():
    """HW = 200 is three chunks of 67, 67, 66: the middle one left out of channel 1's mean"""
    c, f = chatt_fault_case()
    ref = AT.chatt_pool_ref(c['x'])
    AT.check(f['pool'], *ref, AT.KAPPA[('chatt', 'pool')], what='clean')
    x = c['x'].clone()
    x[:, 67:134, 1] = 0
    f2 = AT.chatt_fwd_t(x, c['s'], c['wd'], c['bd'], c['wu'], c['bu'])
    pool = f['pool'].clone(); pool[:, 1] = f2['pool'][:, 1]
    f3 = AT.chatt_fwd_t(c['x'], c['s'], c['wd'], c['bd'], c['wu'], c['bu'])          # ... and what the later stages make of that pool
    hid = torch.relu(pool @ c['wd'].T + c['bd']); a = torch.sigmoid(hid @ c['wu'].T + c['bu'])
    a64, out64 = chatt_end_to_end(c)
    assert old_err(a, a64) <= 2e-6 and old_err((1 + a)[:, None, :] * c['x'] + c['s'], out64) <= 2e-6 and old_err(pool, ref[0]) <= 2e-6
    assert torch.equal(f3['pool'], f['pool'])
    rejected(pool, *ref, ('chatt', 'pool'))


# ---------------------------------------------------------------- KL
def kl_fault_case():
    c = dict(G.kl_case(2, 3, 16, 'row', None, False))
    c['w'] = c['w'].clone()
    c['w'][0] = torch.tensor([0.25e-5, 0.25, 0.25])          # a sample that hardly counts beside two that do
    return c


def test_fault_dpmu_summed_over_one_row_less():
    c = kl_fault_case()
    ref = AT.kl_ref(c['mu'], c['lv'], c['w'], c['pm'], c['plv'], G.G_UP)
    o = AT.kl_t(c['mu'], c['lv'], c['w'], c['pm'], c['plv'], G.G_UP)
    for n in o:
        AT.check(o[n], *ref[n], AT.KAPPA[('kl', n)], what='clean ' + n)
    term = -(G.G_UP * c['w'][0, 0]) * (c['mu'][0, 0] - c['pm'][0]) / torch.exp(c['plv'][0])          # row b = 0 of contrast 0: (Z,)
    z = int((term.double().abs() / ref['dpmu'][1][0]).argmax())
    dpmu = o['dpmu'].clone()
    dpmu[0, z] -= term[z]
    assert old_kl_close(dpmu, ref['dpmu'][0])
    rejected(dpmu, *ref['dpmu'], ('kl', 'dpmu'))


def test_fault_dlv_reads_the_prior_row_of_another_contrast():
    c = kl_fault_case()
    c['plv'] = c['plv'].clone()
    c['plv'][1] = c['plv'][0] + 4e-6          # two contrasts whose learned priors differ slightly
    ref = AT.kl_ref(c['mu'], c['lv'], c['w'], c['pm'], c['plv'], G.G_UP)
    o = AT.kl_t(c['mu'], c['lv'], c['w'], c['pm'], c['plv'], G.G_UP)
    AT.check(o['dlv'], *ref['dlv'], AT.KAPPA[('kl', 'dlv')], what='clean')
    swapped = AT.kl_t(c['mu'], c['lv'], c['w'], c['pm'], c['plv'][[1, 0]], G.G_UP)['dlv']
    dlv = o['dlv'].clone(); dlv[1] = swapped[1]          # contrast 1 read row 0
    assert not torch.equal(dlv, o['dlv']) and old_kl_close(dlv, ref['dlv'][0])
    rejected(dlv, *ref['dlv'], ('kl', 'dlv'))


# ---------------------------------------------------------------- residual gate
def test_fault_rgate_row_clamp_one_short():
    """y1 = y0 + (y0 < h - 2): the output rows between the gate's last two rows read the upper one twice; planted at one pixel of a dark border
    (x a million times smaller than elsewhere)"""
    B, C, h, w = 2, 64, 5, 6
    x, alpha = G.rnd((B, 2 * h, 2 * w, C), 21), G.rnd((B, h, w), 23, 0.7)
    yy, xx = 2 * (h - 2) + 1, 4          # source row h - 2 + 0.25: y0 = h - 2, y1 = h - 1
    x[0, yy, xx] *= 1e-6
    ref = AT.rgate_fwd_ref(x, alpha)
    out = YARD.rgate_fwd(x, alpha, G.DENSE)
    AT.check(out, *ref, AT.KAPPA[('rgate', 'out')], what='clean')
    short = alpha.clone(); short[:, h - 1] = alpha[:, h - 2]
    bad = out.clone(); bad[0, yy, xx] = YARD.rgate_fwd(x, short, G.DENSE)[0, yy, xx]
    assert not torch.equal(bad, out) and old_err(bad, ref[0]) <= 2e-6 / 10
    rejected(bad, *ref, ('rgate', 'out'))


def test_nan_fails_and_exact_zero_is_required():
    g, dgd = G.rnd((1, 3, 2, 4), 1), G.rnd((1, 3, 2, 4), 2)
    ref, A = AT.symdiff_bwd_ref(dgd, g)
    assert not bool(ref[:, 1].any())          # the middle row of an odd H
    got = ref.float().clone(); got[0, 0, 0, 0] = float('nan')
    rejected(got, ref, A, ('symdiff', 'dg'))
    with pytest.raises(AssertionError):
        G.is_zero(torch.tensor([0.0, 1e-30]), 'middle row')
    G.is_zero(torch.tensor([0.0, -0.0]), 'middle row')
