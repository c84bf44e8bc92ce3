"""tests/elem3d_check.py on the CPU: its references agree with float64 autograd through F.group_norm (+ F.relu) and through nearest
F.interpolate; its bound is not vacuous (one wrong element of 64 u A, or one channel quad swapped with its neighbour, in a copy of the reference is
rejected for every checked output, while a plain fp32 torch evaluation passes at the committed kappas); and the condition the GPU rows rely on --
at most AMBIGUOUS_CAP of a row's elements within the forward bound of the ReLU's edge -- holds for every row's seeded inputs."""
import pytest
import torch
import torch.nn.functional as F

import elem3d_check as E3
import test_gpu_elem3d_paths as T

K = E3.KAPPA
EPS = E3.EPS


def f64(shape, g, scale=1.0, mean=0.0):
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale + mean


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('N,C,dhw,G', [(2, 8, (2, 3, 5), 1), (2, 8, (2, 3, 5), 8), (3, 16, (1, 1, 7), 4), (1, 4, (1, 1, 1), 2)])
def test_groupnorm_references_match_autograd(N, C, dhw, G, relu):
    g_ = torch.Generator().manual_seed(5)
    x = f64((N, C) + dhw, g_, 2.0, 0.5).requires_grad_(True)
    gamma = (1 + 0.3 * f64((C,), g_)).requires_grad_(True); beta = (0.2 * f64((C,), g_)).requires_grad_(True)
    dy = f64((N, C) + dhw, g_, 2.0, 0.5)
    y = F.group_norm(x, G, gamma, beta, EPS)
    y = F.relu(y) if relu else y
    dx, dg, db = torch.autograd.grad(y, (x, gamma, beta), dy)
    xd, gd, bd = x.detach(), gamma.detach(), beta.detach()
    close = lambda a, b: torch.allclose(a, b, rtol=1e-12, atol=1e-12 * float(b.abs().max()))
    s = E3.gn_stats_ref(xd, G, EPS)
    xg = xd.reshape(N * G, -1)
    assert close(s['mean'][0], xg.mean(1)) and close(s['var'][0], xg.var(1, unbiased=False)) and s['P'] == xg.shape[1]
    assert (s['mean'][1] >= s['mean'][0].abs()).all() and (s['var'][1] >= s['var'][0]).all()
    ref, A, z = E3.gn_apply_ref(xd, s['mean'][0], s['rstd'], gd, bd, relu)
    assert close(ref, y.detach()) and (A >= z.abs() - 1e-12).all()
    b = E3.gn_bwd_ref(dy, xd, gd, bd, s['mean'][0], s['rstd'], G, relu)
    assert close(b['dx'][0], dx) and close(b['dgamma'][0], dg) and close(b['dbeta'][0], db)
    assert b['share'] == 0.0 and b['mask_disagree'] == 0 and all(float(b[n][2].abs().max()) == 0.0 for n in ('dx', 'dgamma', 'dbeta'))
    assert all((b[n][1] >= b[n][0].abs() - 1e-12).all() for n in ('dx', 'dgamma', 'dbeta'))
    # the mask is an input: with the stored y > 0 of a forward that zeroed everything, the gradient is that of a dead layer
    if relu:
        dead = E3.gn_bwd_ref(dy, xd, gd, bd, s['mean'][0], s['rstd'], G, relu, mask=torch.zeros_like(xd, dtype=torch.bool))
        assert float(dead['dx'][0].abs().max()) == 0.0 and dead['mask_disagree'] == int((z > 0).sum())


@pytest.mark.parametrize('geom', [(2, 4, 3, 5, 4), (1, 4, 1, 1, 1), (2, 8, 1, 7, 1), (1, 12, 5, 1, 3)])
def test_upsampling_references_match_autograd(geom):
    N, C, D, H, W = geom
    g_ = torch.Generator().manual_seed(6)
    x = f64(geom, g_).requires_grad_(True)
    skip = f64((N, C, 2 * D, 2 * H, 2 * W), g_); dy = f64((N, C, 2 * D, 2 * H, 2 * W), g_)
    y = F.interpolate(x, scale_factor=2, mode='nearest')
    dx, = torch.autograd.grad(y, x, dy)
    assert torch.equal(E3.up2_ref(x.detach()), y.detach()) and torch.equal(E3.up2_ref(x.detach(), skip), y.detach() + skip)
    assert torch.allclose(E3.up2_bwd_ref(dy), dx, rtol=1e-12, atol=1e-12)
    # the documented order: depth offset, then height, then width -- and no other (fp32, where the order shows in the bits)
    d32 = (dy * 1e3).float()
    seq = torch.zeros(geom)
    for k in range(8):
        seq = seq + d32[:, :, (k >> 2)::2, ((k >> 1) & 1)::2, (k & 1)::2]
    E3.assert_same_bits(E3.up2_bwd_ref(d32), seq, 'up2_bwd_ref')


ROW = dict(id='cpu', N=2, C=16, dhw=(3, 5, 7), G=4, relu=1, mean=0.5)


def fp32_outputs(row):
    """a plain fp32 torch evaluation of the row (the yardstick of the GPU test) and the float64 references of every checked output"""
    inp = E3.gn_inputs(row)
    x, G = inp['x'], row['G']
    xg = x.reshape(row['N'] * G, -1)
    got = dict(mean=xg.mean(1), rstd=(xg.var(1, unbiased=False) + EPS).rsqrt())
    s = E3.gn_stats_ref(x, G, EPS)
    mask = T.gn_yardstick(inp, row, got, torch.ones_like(x, dtype=torch.bool))['y apply'] > 0          # (the forward does not read the mask)
    yd = T.gn_yardstick(inp, row, got, mask)
    b = E3.gn_bwd_ref(inp['dy'], x, inp['gamma'], inp['beta'], got['mean'], got['rstd'], G, row['relu'], mask=mask, k_apply=K[('gn', 'y apply')], k_sum=K[('gn', 'sums')])
    out = {'mean': (got['mean'], *s['mean'], None), 'var': (E3.var_from_rstd(got['rstd'], EPS), *s['var'], E3.rstd_rounding(s['var'][0], EPS))}
    ref, A, _ = E3.gn_apply_ref(x, got['mean'], got['rstd'], inp['gamma'], inp['beta'], row['relu'])
    out['y apply'] = (yd['y apply'], ref, A, None)
    ref, A, _ = E3.gn_apply_ref(x, s['mean'][0], s['rstd'], inp['gamma'], inp['beta'], row['relu'])
    out['y'] = (yd['y'], ref, A, E3.gn_stats_propagated(x, s, inp['gamma'], K[('gn', 'mean')], K[('gn', 'var')], EPS))
    for n in ('dbeta', 'dgamma', 'dx'):
        out[n] = (yd[n], *b[n])
    return out, b


def test_bound_passes_fp32_and_rejects_planted_faults():
    out, b = fp32_outputs(ROW)
    assert b['mask_disagree'] == 0 and b['share'] <= E3.AMBIGUOUS_CAP
    for name, (got, ref, A, extra) in out.items():
        k = K[('gn', name)]
        E3.check(got, ref, A, k, 0.0, extra, what=name)          # the clean fp32 evaluation is inside the bound
        # one wrong element of 64 u A, where A is largest
        i = int(A.reshape(-1).argmax())
        bad = ref.clone().reshape(-1)
        bad[i] += 64 * E3.U * float(A.reshape(-1)[i])
        with pytest.raises(AssertionError):
            E3.check(bad.reshape(ref.shape), ref, A, k, 0.0, extra, what=f'{name}: one element off by 64 u A')
        # one channel quad swapped with the next (the statistics: one group's value with the next group's)
        bad = ref.clone()
        if bad.dim() == 5:
            bad[1, 4:8, 2, 3, 4], bad[1, 8:12, 2, 3, 4] = ref[1, 8:12, 2, 3, 4], ref[1, 4:8, 2, 3, 4]
        elif name in ('mean', 'var'):
            bad[5], bad[6] = ref[6], ref[5]
        else:
            bad[4:8], bad[8:12] = ref[8:12], ref[4:8]
        with pytest.raises(AssertionError):
            E3.check(bad, ref, A, k, 0.0, extra, what=f'{name}: swapped quad')


@pytest.mark.parametrize('row', [pytest.param(r, id=r['id']) for r in E3.GN_ROWS])
def test_ambiguous_share_of_every_gpu_row(row):
    """from the float64 reference alone (its statistics rounded to fp32, as a kernel returns them): the share of elements within the forward bound of
    the ReLU's edge stays under the cap the GPU rows assert -- about 1e-5 at the usual mean, more where |mean| >> sigma makes A large"""
    inp = E3.gn_inputs(row)
    s = E3.gn_stats_ref(inp['x'], row['G'], EPS)
    mean, rstd = s['mean'][0].float(), s['rstd'].float()
    b = E3.gn_bwd_ref(inp['dy'], inp['x'], inp['gamma'], inp['beta'], mean, rstd, row['G'], row['relu'], k_apply=K[('gn', 'y apply')], k_sum=K[('gn', 'sums')])
    print(f"ambiguous share {b['share']:.2e}  ({row['id']})")
    assert b['share'] <= E3.AMBIGUOUS_CAP and b['mask_disagree'] == 0
    if not row['relu']:
        assert b['share'] == 0.0


def test_every_output_has_a_kappa():
    assert {k[1] for k in K} == {'mean', 'var', 'y apply', 'y', 'dbeta', 'dgamma', 'dx', 'sums'} and all(k[0] == 'gn' and v >= 1 for k, v in K.items())
