"""The element-wise float64 bound of tests/elem_check.py against the max-scaled close() of tests/test_gpu_ops.py, on the CPU: each operation is
emulated in fp32 the way its kernel computes it (fp32 partial sums over chunks of rows combined in float64, fp32 apply expressions), the clean
emulation passes the bound at the kappa committed for the kernel, and one planted fault -- confined to a low-amplitude channel, as a wrong lane
mask or a mis-indexed statistic would be -- is rejected by the bound while close() passes it at the rtol the suite uses for that result."""
import pytest
import torch
import torch.nn.functional as F

import elem_check as EC
from test_gpu_ops import close

K = EC.KAPPA
EPS, MOM = 1e-5, 0.1
LOW = 3            # the channel that carries the fault: its data and / or its gamma are 1000 x smaller than the others'


def rnd(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def layer(P, C=8, seed=0, low_x=1e-3):
    """x (1, C, 1, P) fp32 = randn * 2 + 0.5 with channel LOW scaled by low_x; gamma with gamma[LOW] scaled by 1e-3; beta; dy"""
    x = rnd((1, C, 1, P), seed, 2.0) + 0.5
    x[:, LOW] *= low_x
    gamma = rnd((C,), seed + 1) + 1.5
    gamma[LOW] *= 1e-3
    return x, gamma, rnd((C,), seed + 2) * 0.1, rnd((1, C, 1, P), seed + 3, 2.0) + 0.5


def chunk_sums(x, rpb, skip=None, drop_last_row_of=None):
    """fp32 sums of x and x^2 over chunks of rpb rows, combined in float64 (stat_partial_kernel + stat_final_kernel); skip = (chunk, channel)
    leaves that chunk out of that channel's sums; drop_last_row_of = channel: the last row of the (ragged) last chunk is not read"""
    rows = x[0, :, 0, :].t().contiguous()          # (P, C)
    P, C = rows.shape
    s0 = torch.zeros(C, dtype=torch.float64); s1 = torch.zeros(C, dtype=torch.float64)
    for k, r0 in enumerate(range(0, P, rpb)):
        blk = rows[r0:r0 + rpb].clone()
        if drop_last_row_of is not None and r0 + rpb >= P:
            blk[-1, drop_last_row_of] = 0
        a, b = blk.sum(0).double(), (blk * blk).sum(0).double()
        if skip is not None and skip[0] == k:
            a[skip[1]] = 0; b[skip[1]] = 0
        s0 += a; s1 += b
    return s0, s1, P


def finish(s0, s1, P):
    m = s0 / P
    var = (s1 / P - m * m).clamp_min(0)
    return m.float(), ((var + EPS) ** -0.5).float(), m, var


def check_stats(x, mean, rstd, fam='stat_vec'):
    st = EC.stats_ref(x, 1, EPS)
    EC.check(mean, *st['mean'], K[(fam, 'mean')], what='mean')
    EC.check(EC.var_from_rstd(rstd, EPS), *st['var'], K[(fam, 'var')], extra=EC.rstd_rounding(st['var'][0], EPS), what='var')
    return st


@pytest.mark.parametrize('fault', [None, 'chunk', 'row'])
def test_statistics_chunk_of_33_left_out_and_last_row_of_a_ragged_chunk(fault):
    P = 33 * 256 if fault != 'row' else 257
    x, gamma, beta, _ = layer(P)
    rpb = 256 if fault != 'row' else 129
    s0, s1, _ = chunk_sums(x, rpb, skip=(17, LOW) if fault == 'chunk' else None, drop_last_row_of=LOW if fault == 'row' else None)
    mean, rstd, _, _ = finish(s0, s1, P)
    y = (x - mean.view(1, -1, 1, 1)) * (rstd * gamma).view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
    if fault is None:
        st = check_stats(x, mean, rstd)
        EC.check(y, *EC.norm_apply_ref(x, mean, rstd, 1, gamma, beta), K[('bn', 'y apply')], what='y apply')
        EC.check(y, *EC.norm_apply_ref(x, st['mean'][0], st['rstd'], 1, gamma, beta), K[('bn', 'y')],
                 extra=EC.stats_propagated(x, st, 1, gamma, K[('stat_vec', 'mean')], K[('stat_vec', 'var')], EPS), what='y')
        return
    xd = x.double()
    close(mean, xd.mean((0, 2, 3)), rtol=1e-4, what='close() passes the faulty mean')
    close(y, F.batch_norm(xd, None, None, gamma.double(), beta.double(), True, 0.0, EPS), rtol=1e-4, what='close() passes the faulty y')
    with pytest.raises(AssertionError):
        check_stats(x, mean, rstd)
    st = EC.stats_ref(x, 1, EPS)
    with pytest.raises(AssertionError):          # end to end, the propagated statistics bound does not hide it either
        EC.check(y, *EC.norm_apply_ref(x, st['mean'][0], st['rstd'], 1, gamma, beta), K[('bn', 'y')],
                 extra=EC.stats_propagated(x, st, 1, gamma, K[('stat_vec', 'mean')], K[('stat_vec', 'var')], EPS), what='y')


def run_update(rm0, rv0, m, var, P, unbiased=True, round_between=True):
    """the running statistics after the groups' (m, var) (float64, (G, C)) as stat_final_kernel / stat_final_groups_kernel form them"""
    rm, rv = rm0.double(), rv0.double()
    for g in range(m.shape[0]):
        unb = var[g] * P / (P - 1) if unbiased and P > 1 else var[g]
        rm = (1 - MOM) * rm + MOM * m[g]; rv = (1 - MOM) * rv + MOM * unb
        if round_between:
            rm, rv = rm.float().double(), rv.float().double()
    return rm.float(), rv.float()


def test_running_var_without_the_unbiased_factor():
    P = 65 * 256
    x, _, _, _ = layer(P)
    rm0, rv0 = rnd((8,), 5), rnd((8,), 6).abs() + 0.5
    rv0[0] = 3.0
    s0, s1, _ = chunk_sums(x, 256)
    _, _, m, var = finish(s0, s1, P)
    st = EC.stats_ref(x, 1, EPS)
    r_rm, A_rm, r_rv, A_rv = EC.running_ref(rm0, rv0, st['mean'][0], st['var'][0], st['mean'][1], st['var'][1], P, MOM, 1)
    rm, rv = run_update(rm0, rv0, m[None], var[None], P)
    EC.check(rm, r_rm, A_rm, K[('stat_vec', 'run_mean')], what='running_mean'); EC.check(rv, r_rv, A_rv, K[('stat_vec', 'run_var')], what='running_var')
    _, rv_bad = run_update(rm0, rv0, m[None], var[None], P, unbiased=False)
    close(rv_bad, r_rv, rtol=1e-5, what='close() passes the biased running_var')
    with pytest.raises(AssertionError):
        EC.check(rv_bad, r_rv, A_rv, K[('stat_vec', 'run_var')], what='running_var')
    # P == 1 stays biased
    x1 = rnd((1, 8, 1, 1), 9)
    st1 = EC.stats_ref(x1, 1, EPS)
    _, _, r1, _ = EC.running_ref(rm0, rv0, st1['mean'][0], st1['var'][0], st1['mean'][1], st1['var'][1], 1, MOM, 1)
    assert torch.equal(r1, ((1 - MOM) * rv0.double()).float().double())


def test_grouped_running_statistics_not_rounded_between_groups():
    """a half-ulp matter: inside any bound with kappa >= 1 and inside close(); the grouped form is held to the BITS of G separate calls"""
    G, P = 4, 257
    xs = [layer(P, seed=10 * g)[0] for g in range(G)]
    rm0, rv0 = rnd((8,), 5), rnd((8,), 6).abs() + 0.5
    stats = [finish(*chunk_sums(x, 129)) for x in xs]
    m, var = torch.stack([s[2] for s in stats]), torch.stack([s[3] for s in stats])
    rm_seq, rv_seq = rm0, rv0
    for g in range(G):          # G separate calls
        rm_seq, rv_seq = run_update(rm_seq, rv_seq, m[g:g + 1], var[g:g + 1], P)
    rm, rv = run_update(rm0, rv0, m, var, P)
    EC.assert_same_bits(rm, rm_seq, 'running_mean'); EC.assert_same_bits(rv, rv_seq, 'running_var')
    x = torch.cat(xs, 0)
    st = EC.stats_ref(x, G, EPS)
    r_rm, A_rm, r_rv, A_rv = EC.running_ref(rm0, rv0, st['mean'][0], st['var'][0], st['mean'][1], st['var'][1], P, MOM, G)
    EC.check(rm, r_rm, A_rm, K[('stat_vec', 'run_mean')], what='running_mean'); EC.check(rv, r_rv, A_rv, K[('stat_vec', 'run_var')], what='running_var')
    differs = False
    for seed in range(8):       # unrounded between the groups: some seed's result differs in its last bit from the separate calls
        rm0, rv0 = rnd((8,), 50 + seed), rnd((8,), 60 + seed).abs() + 0.5
        rm_seq, rv_seq = rm0, rv0
        for g in range(G):
            rm_seq, rv_seq = run_update(rm_seq, rv_seq, m[g:g + 1], var[g:g + 1], P)
        rm_bad, rv_bad = run_update(rm0, rv0, m, var, P, round_between=False)
        close(rm_bad, rm_seq, rtol=1e-5); close(rv_bad, rv_seq, rtol=1e-5)
        if not (torch.equal(rm_bad, rm_seq) and torch.equal(rv_bad, rv_seq)):
            differs = True
            with pytest.raises(AssertionError):
                EC.assert_same_bits(torch.cat([rm_bad, rv_bad]), torch.cat([rm_seq, rv_seq]), 'unrounded')
    assert differs


def test_dx_with_the_neighbouring_channels_rstd():
    P = 257
    x, gamma, _, dy = layer(P, low_x=1.0)          # (dx scales with gamma rstd: only gamma is small here)
    mean, rstd, _, _ = finish(*chunk_sums(x, 129))
    m, r, g = mean.view(1, -1, 1, 1), rstd.view(1, -1, 1, 1), gamma.view(1, -1, 1, 1)
    xh = (x - m) * r
    sdy, sdyxh = dy.sum((0, 2, 3)), (dy * xh).sum((0, 2, 3))
    s0, A0, s1, A1 = EC.bwd_sums_ref(dy, x, mean, rstd, 1)
    EC.check(sdy, s0, A0, K[('stat_vec', 'dbeta')], what='sum dy'); EC.check(sdyxh, s1, A1, K[('stat_vec', 'dgamma')], what='sum dy xhat')

    def dx_of(rr):
        inv = torch.tensor(1.0 / P)
        return g * rr * (dy - sdy.view(1, -1, 1, 1) * inv - ((x - m) * rr) * sdyxh.view(1, -1, 1, 1) * inv)
    ref, A = EC.bwd_apply_ref(dy, x, mean, rstd, 1, sdy, sdyxh, P, gamma=gamma)
    EC.check(dx_of(r), ref, A, K[('bn', 'dx')], what='dx')
    r_bad = r.clone(); r_bad[:, LOW] = r[:, LOW + 1]          # the neighbour's statistic: a few per cent off (two samples of the same distribution)
    close(dx_of(r_bad), ref, rtol=1e-4, what='close() passes the faulty dx')
    with pytest.raises(AssertionError):
        EC.check(dx_of(r_bad), ref, A, K[('bn', 'dx')], what='dx')


def test_x2_adjoint_border_row_with_the_interior_weights():
    N, C, Hi, Wi = 1, 8, 5, 7
    dy = rnd((N, C, 2 * Hi, 2 * Wi), 1, 2.0) + 0.5
    dy[:, LOW] *= 1e-4
    ref, A = EC.bilinear_bwd_ref(dy, (Hi, Wi), False)
    x = torch.zeros((N, C, Hi, Wi), requires_grad=True)
    got, = torch.autograd.grad(F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False), x, dy)
    EC.check(got, ref, A, K[('bil_bwd_x2', 'dx')], what='x2 adjoint')
    # row 0 of dx takes output row 0 with weight 1.0 (0.75 + the clamped 0.25); the interior weights give it 0.75
    top = torch.zeros_like(dy); top[:, :, 0] = dy[:, :, 0]
    lost = 0.25 * EC.bilinear_bwd_ref(top, (Hi, Wi), False)[0][:, LOW, 0]
    bad = got.clone().double(); bad[:, LOW, 0] -= lost
    close(bad, ref, rtol=1e-5, what='close() passes the faulty border row')
    with pytest.raises(AssertionError):
        EC.check(bad, ref, A, K[('bil_bwd_x2', 'dx')], what='x2 adjoint')


def test_resize_dx_without_the_last_output_column():
    N, C, Hi, Wi, Ho, Wo = 1, 8, 7, 9, 13, 20
    dy = rnd((N, C, Ho, Wo), 1, 2.0) + 0.5
    dy[:, LOW] *= 1e-5
    for align in (False, True):
        ref, A = EC.bilinear_bwd_ref(dy, (Hi, Wi), align)
        ex = EC.bilinear_bwd_index_extra(dy, (Hi, Wi), align)          # (a general resize: the fp32 source index)
        x = torch.zeros((N, C, Hi, Wi), requires_grad=True)
        got, = torch.autograd.grad(F.interpolate(x, size=(Ho, Wo), mode='bilinear', align_corners=align), x, dy)
        EC.check(got, ref, A, K[('bil_bwd_general', 'dx')], extra=ex, what='resize adjoint')
        last = torch.zeros_like(dy); last[:, LOW, :, -1] = dy[:, LOW, :, -1]
        bad = got.double() - EC.bilinear_bwd_ref(last, (Hi, Wi), align)[0]
        close(bad, ref, rtol=1e-5, what='close() passes the missing column')
        with pytest.raises(AssertionError):
            EC.check(bad, ref, A, K[('bil_bwd_general', 'dx')], extra=ex, what='resize adjoint')


def test_spade_up2_reference_matches_autograd():
    """with exact statistics, U^T of the instance-norm backward is autograd through interpolate -> instance_norm -> modulation; A bounds |ref|"""
    g_ = torch.Generator().manual_seed(3)
    for (N, C, Hi, Wi) in [(2, 4, 9, 15), (1, 8, 1, 11)]:
        x = (torch.randn(N, C, Hi, Wi, generator=g_, dtype=torch.float64) * 2 + 0.5).requires_grad_(True)
        g = torch.randn(N, C, 2 * Hi, 2 * Wi, generator=g_, dtype=torch.float64); d = torch.randn(N, C, 2 * Hi, 2 * Wi, generator=g_, dtype=torch.float64)
        z = F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False)
        zd = z.detach()
        gg = g.clone().requires_grad_(True)
        out = F.instance_norm(z, eps=EPS) * (1 + g)
        dx, = torch.autograd.grad(out, x, d)
        st = EC.stats_ref(zd, N, EPS)
        r = EC.spade_bwd_up2_ref(d, x.detach(), g, st['mean'][0], st['rstd'], 1.0)
        assert torch.allclose(r['dx'][0], dx, rtol=1e-9, atol=1e-11)
        assert (r['dx'][1] >= r['dx'][0].abs() - 1e-12).all() and (r['dx'][2] >= 0).all()
        dgam, = torch.autograd.grad(F.instance_norm(zd, eps=EPS) * (1 + gg), gg, d)
        assert torch.allclose(r['dgamma'][0], dgam, rtol=1e-9, atol=1e-11)


def test_bn_and_spade_references_match_autograd():
    g_ = torch.Generator().manual_seed(4)
    x = (torch.randn(4, 5, 3, 7, generator=g_, dtype=torch.float64) * 2 + 0.5).requires_grad_(True)
    gamma = torch.randn(5, generator=g_, dtype=torch.float64); beta = torch.randn(5, generator=g_, dtype=torch.float64); dy = torch.randn(4, 5, 3, 7, generator=g_, dtype=torch.float64)
    for G in (1, 2):
        xg = x.reshape(G, 4 // G, 5, 3, 7)
        y = torch.cat([F.batch_norm(xg[i], None, None, gamma, beta, True, 0.0, EPS) for i in range(G)], 0)
        dx, = torch.autograd.grad(y, x, dy)
        st = EC.stats_ref(x.detach(), G, EPS)
        P = st['P']
        ref, A = EC.norm_apply_ref(x.detach(), st['mean'][0], st['rstd'], G, gamma, beta)
        assert torch.allclose(ref, y.detach()) and (A >= ref.abs() - 1e-12).all()
        s0, A0, s1, A1 = EC.bwd_sums_ref(dy, x.detach(), st['mean'][0], st['rstd'], G)
        rdx, Adx = EC.bwd_apply_ref(dy, x.detach(), st['mean'][0], st['rstd'], G, s0, s1, P, gamma=gamma)
        assert torch.allclose(rdx, dx) and (Adx >= rdx.abs() - 1e-12).all() and (A0 >= s0.abs()).all() and (A1 >= s1.abs() - 1e-12).all()
    bn = torch.nn.BatchNorm2d(5, eps=EPS, momentum=MOM).double().train()
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    for i in range(2):
        bn(x.detach()[2 * i:2 * i + 2])
    st = EC.stats_ref(x.detach(), 2, EPS)
    rm, _, rv, _ = EC.running_ref(rm0, rv0, st['mean'][0], st['var'][0], st['mean'][1], st['var'][1], st['P'], MOM, 2)
    assert torch.allclose(rm, bn.running_mean, rtol=1e-6) and torch.allclose(rv, bn.running_var, rtol=1e-6)          # (the reference rounds to fp32 between calls)
