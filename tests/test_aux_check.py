"""tests/aux_check.py on the CPU: faults planted into a correct fp32 result -- what a wrong tile mask, a swapped tap, a double-counted type, a wrong step
count, a leaking gate, an unclamped clip, a late argmax, a truncating cast or a mis-indexed gather would produce -- are rejected by the checks of
tests/test_gpu_aux_paths.py, each by name; the plain fp32 torch evaluation of every row of that suite (its TorchImpl: the yardstick) passes its own
bound and every exact assertion; and aux_check.KAPPA is what the yardsticks say: 4 x the worst ratio of the operation's rows, at least 1."""
import math

import pytest
import torch

import aux_check as AC
import test_gpu_aux_paths as G

F32, B16 = torch.float32, torch.bfloat16
YARD = G.TorchImpl()


def rejected(got, ref, A, key, **kw):
    with pytest.raises(AssertionError):
        AC.check(got, ref, A, AC.KAPPA[key], what='planted fault', **kw)


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
    bad = [(rid, name, key, r) for rid, items in yardsticks.items() for name, key, r in items if not r <= AC.KAPPA[key]]
    assert not bad, bad


def test_kappa_is_four_times_the_worst_yardstick(yardsticks):
    worst = {}
    for items in yardsticks.values():
        for _, key, r in items:
            worst[key] = max(worst.get(key, 0.0), r)
    assert set(worst) == set(AC.KAPPA), set(worst) ^ set(AC.KAPPA)
    # the rule is 4 x the worst yardstick SEEN: fp32 torch rounds a little differently from CPU to CPU (FMA contraction, how many threads a sum is split
    # over; up to 13 % between two evaluations of these rows), so the table is held to ceil(4 w) with 15 % of slack on w either way
    for key, w in worst.items():
        assert AC.KAPPA[key] >= 1 and 4.0 * w / 1.15 <= AC.KAPPA[key] <= max(1, math.ceil(4.0 * w * 1.15)), (key, w, AC.KAPPA[key])


# ---------------------------------------------------------------- expert mixing
@pytest.fixture(scope='module')
def mix():
    c = G.mix_case(3, 4, 40, 24, 9, 1, (True, False, True, True))
    ref = G.mix_refs(c)
    f = YARD.mix_fwd(c)
    return c, ref, f, YARD.mix_bwd(c, f)


def test_fault_one_expert_dropped_on_one_tile(mix):
    c, ref, f, _ = mix
    m, e = 2, 1
    w = AC.from_tck(f['tck'][m]).clone()
    AC.check(AC.to_tck(w), AC.to_tck(ref['w'][0][m]), AC.to_tck(ref['w'][1][m]), AC.KAPPA[('mix', 'w')], what='clean')
    w[:32, :8] -= f['r'][m, e] * c['W'][e, :32, :8]          # one 32 x 8 (cout, channel) tile
    rejected(AC.to_tck(w), AC.to_tck(ref['w'][0][m]), AC.to_tck(ref['w'][1][m]), ('mix', 'w'))


def test_fault_two_taps_swapped(mix):
    c, ref, f, _ = mix
    t = f['tck'][0].clone()
    t[[3, 4]] = t[[4, 3]]
    rejected(t, AC.to_tck(ref['w'][0][0]), AC.to_tck(ref['w'][1][0]), ('mix', 'w'))


def test_fault_one_types_gradient_added_twice(mix):
    c, ref, f, b = mix
    AC.check(b['dW'], *ref['dW'], AC.KAPPA[('mix', 'dW')], what='clean')
    dW = b['dW'] + f['r'][3][:, None, None, None] * AC.from_tck(c['dws'][3])[None]
    rejected(dW, *ref['dW'], ('mix', 'dW'))
    # ... and in the routing gradients, whose scale is the sum over the types
    twice = list(c['dws']); twice[3] = 2 * c['dws'][3]
    g2 = AC.mix_routing_grad_ref(c['W'], c['fcw'], c['fcb'], c['types'], twice, dtype=F32)
    rejected(g2['dfcb'][0], *ref['dfcb'], ('mix', 'dfcb')); rejected(g2['dfcw'][0], *ref['dfcw'], ('mix', 'dfcw'))


def test_fault_gradient_of_an_absent_type_read(mix):
    """m = 1 has no gradient: a body that reads type 0's in its place"""
    c, ref, f, b = mix
    dW = b['dW'] + f['r'][1][:, None, None, None] * AC.from_tck(c['dws'][0])[None]
    rejected(dW, *ref['dW'], ('mix', 'dW'))


# ---------------------------------------------------------------- optimizer arena: the arena rule restated in fp32, with switches for the faults
def arena_adam(s, count=None, gated_off_moves=False, clip_unclamped=False, bc_fp32=False):
    count = count or ('own' if s['own_counts'] else 'arena')
    h = {k: torch.tensor(AC.f32(v), dtype=F32) for k, v in s['hyper'].items()}
    n = s['p0'].numel()
    p = s['p0'].clone(); m, v, vm = torch.zeros(n), torch.zeros(n), torch.zeros(n)
    n_flags = (max(s['fidx']) + 1) if s['fidx'] else 0
    arena, gsteps = 0, [0] * n_flags
    for k, g in enumerate(s['grads']):
        if s['norm'] and not bool(torch.isfinite(g).all()):
            continue
        arena += 1
        coef = h['grad_scale']
        if s['norm'] and float(h['max_norm']) > 0:
            cc = h['max_norm'] / ((g * g).sum().sqrt() * h['grad_scale'] + 1e-6)
            coef = h['grad_scale'] * (cc if clip_unclamped else cc.clamp(max=1.0))
        t = torch.full((n,), float(arena)); on = torch.ones(n, dtype=torch.bool)
        for f in range(n_flags):
            gsteps[f] += int(s['flags'][k][f] != 0)
        for (lo, hi), f in zip(s['ranges'], s['fidx']):
            if count == 'own':
                t[lo:hi] = gsteps[f]
            if not s['flags'][k][f] and not gated_off_moves:
                on[lo:hi] = False
        t = t.clamp(min=1).double()
        if bc_fp32:          # 1.f - powf(b, t) as the kernel forms it: the subtraction cancels (1 - 0.999^t is ~t / 1000) and the rounding of the power stays
            bc1, sbc2 = 1 - h['b1'] ** t.float(), (1 - h['b2'] ** t.float()).sqrt()
        else:
            bc1, sbc2 = (1 - float(h['b1']) ** t).float(), (1 - float(h['b2']) ** t).sqrt().float()
        gv = g * coef + h['wd'] * p
        mv = h['b1'] * m + (1 - h['b1']) * gv
        vv = h['b2'] * v + (1 - h['b2']) * gv * gv
        vmv = torch.maximum(vm, vv)
        pv = p - (h['lr'] / bc1) * mv / (vmv.sqrt() / sbc2 + h['eps'])
        p, m, v, vm = (torch.where(on, a, b) for a, b in ((pv, p), (mv, m), (vv, v), (vmv, vm)))
    return dict(p=p, m=m, v=v, vmax=vm)


def adam_row(rid):
    row = next(p.values[0] for p in G.ADAM_ROWS if p.id == rid)
    s = G.adam_spec(row)
    return s, AC.adam_ref(s['p0'], s['grads'], s['flags'], s['ranges'], s['fidx'], clip=s['norm'], arena_count=not s['own_counts'], **s['hyper'])


@pytest.mark.parametrize('rid', [p.id for p in G.ADAM_ROWS])
def test_arena_rule_in_fp32_passes(rid):
    s, ref = adam_row(rid)
    o = arena_adam(s)
    for name in ('p', 'm', 'v', 'vmax'):
        AC.check(o[name], *ref[name], AC.KAPPA[('adam', name)], what=f'{rid}: {name}')


def test_fp32_bias_corrections_are_what_adam_p_spends_its_margin_on():
    """the arena forms 1 - beta^t in fp32 (torch: in double on the host).  Restated with that one change the rule needs about three times the kappa of
    the same rule with exact corrections -- on p only, and still inside the committed one: where the kernels' ratio for p sits (profiles/aux_path_margins.txt)"""
    s, ref = adam_row('adam n10007 max_norm 0 no clip')
    exact, fp32 = arena_adam(s), arena_adam(s, bc_fp32=True)
    r_exact, r_fp32 = (AC.ratio(o['p'], *ref['p']) for o in (exact, fp32))
    assert 2.0 * r_exact < r_fp32 <= AC.KAPPA[('adam', 'p')], (r_exact, r_fp32)
    for name in ('m', 'v', 'vmax'):
        AC.assert_same_bits(fp32[name], exact[name], name)


def test_fault_gate_range_stepped_with_the_arenas_count():
    s, ref = adam_row('adam n10007 two ranges two flags')
    o = arena_adam(s, count='arena')
    rejected(o['p'], *ref['p'], ('adam', 'p'))
    lo, hi = s['ranges'][1]
    bad = (o['p'].double() - ref['p'][0]).abs() > AC.KAPPA[('adam', 'p')] * AC.U * ref['p'][1]
    assert float(bad[lo:hi].float().mean()) > 0.9 and not bool(bad[1:lo].any())          # nearly every element of the range, and none of the ungated rest
    for name in ('m', 'v', 'vmax'):          # (the moments do not see the count)
        AC.check(o[name], *ref[name], AC.KAPPA[('adam', name)], what=name)


def test_fault_gated_off_range_moved():
    s, ref = adam_row('adam n10007 two ranges two flags')
    o = arena_adam(s, gated_off_moves=True)
    for name in ('p', 'm', 'v'):
        rejected(o[name], *ref[name], ('adam', name))


def test_fault_clip_applied_below_max_norm():
    s, ref = adam_row('adam n257 norm below max_norm')
    o = arena_adam(s, clip_unclamped=True)
    for name in ('m', 'v', 'vmax'):
        rejected(o[name], *ref[name], ('adam', name))


def test_fault_skipped_step_applied():
    s, ref = adam_row('adam n257 skipped step in the middle')
    s2 = dict(s); s2['grads'] = [torch.nan_to_num(g) for g in s['grads']]
    o = arena_adam(s2)
    for name in ('p', 'm', 'v'):
        rejected(o[name], *ref[name], ('adam', name))


def test_sumsq_fault_one_block_lost():
    g = G.rnd((G.BIG_N,), 50, 3.0)
    ref, A, _ = AC.sumsq_ref(g)
    AC.check((g ** 2).sum().reshape(1), ref, A, AC.KAPPA[('sumsq', 'sum')], what='clean')
    rejected((g[256:] ** 2).sum().reshape(1), ref, A, ('sumsq', 'sum'))


# ---------------------------------------------------------------- helpers
def test_softmax_fault_mask_logit_not_dropped_from_the_sum():
    s = G.rnd((257, 4), 70, 3.0); mask = (torch.arange(257) % 3 != 0).float()
    ref, A, extra = AC.softmax_md_ref(s, mask, 100.0)
    AC.check(AC.softmax_md_ref(s, mask, 100.0, dtype=F32)[0], ref, A, AC.KAPPA[('softmax', 'out')], extra=extra, what='clean')
    rejected(torch.softmax(s, 1), ref, A, ('softmax', 'out'), extra=extra)          # the mask logit left out of the denominator
    got = ref.float().clone(); got[3, 3] *= 1 + 1e-4                                  # one element, far below what a max-scaled bound sees
    rejected(got, ref, A, ('softmax', 'out'), extra=extra)


def test_recon_fault_last_chunk_lost():
    gt, x, w = G.recon_case(2, 647, 19)
    for p in (1, 2):
        ref, A = AC.recon_err_ref(gt, x, p)
        d = (gt - x).reshape(2, -1)[:, :-5]          # the ragged tail of the last chunk
        got = (d.abs() if p == 1 else d * d).sum(1) / (647 * 19)
        rejected(got, ref, A, ('recon', 'err'))
        dref, dA = AC.recon_err_bwd_ref(gt, x, w, p)
        rejected(-dref.float(), dref, dA, ('recon', 'dx'))          # the sign of gt - x instead of x - gt


def test_fault_argmax_points_at_the_second_of_two_equal_maxima():
    x = G.rnd((1, 2, 4, 4), 90)
    x[0, 0, 0, 0] = x[0, 0, 1, 1] = 9.0
    y, arg = AC.maxpool_ref(x, 2)
    assert int(arg[0, 0, 0, 0]) == 0          # the first in scan order
    late = arg.clone(); late[0, 0, 0, 0] = 1 * 4 + 1
    with pytest.raises(AssertionError):
        G.int_eq(late, arg, 'argmax')
    dy = G.rnd(tuple(y.shape), 91)
    with pytest.raises(AssertionError):          # ... and the gradient lands on the wrong pixel
        G.bits_eq(AC.maxpool_bwd_ref(dy, late, x.shape), AC.maxpool_bwd_ref(dy, arg, x.shape), 'dx')


def test_fault_cast_truncates_instead_of_rounding_to_nearest_even():
    x = G.cast_values((2, 8, 5, 7), F32)
    ref = AC.cast_view_ref(x, B16, 8)
    trunc = (x.view(torch.int32) & -65536).view(F32).to(B16)          # (exact: the dropped bits are zero)
    with pytest.raises(AssertionError):
        G.bits_eq(trunc, ref, 'cast_view')
    up = x.clone(); i = up.view(torch.int32); i += 0x8000             # round half up: wrong only on the ties whose kept mantissa is even
    with pytest.raises(AssertionError):
        G.bits_eq((i & -65536).view(F32)[torch.isfinite(x)].to(B16), ref[torch.isfinite(x)], 'cast_view')
    assert torch.equal(AC.bf16_round(x[torch.isfinite(x)]), ref[torch.isfinite(x)].double())          # the two references agree


def test_fault_gather_one_slice_off():
    H, W, D, block = 3, 4, 10, 3
    vols = [[G.rnd((D, H, W), 7 + m) for m in range(2)]]
    want = AC.slice_gather_ref(vols, [4], [-1], H, W, D, block)
    got = AC.slice_gather_ref(vols, [5], [-1], H, W, D, block)
    with pytest.raises(AssertionError):
        G.bits_eq(got[0], want[0], 'inputs')
    assert torch.equal(want[0][0, 0], vols[0][0][1]) and torch.equal(want[0][0, 7 + 6], vols[0][1][7])          # channel m * 7 + k is slice s - block + k


def test_nan_fails_and_tiny_outputs_pass():
    ref, A, extra = AC.softmax_md_ref(torch.tensor([[-80.0, -30.0]]), torch.ones(1), 100.0)
    AC.check(torch.zeros(1, 2), ref, A, 1, extra=extra, what='underflow')          # e^-180 and e^-130: both below the smallest normal fp32
    got = ref.float().clone(); got[0, 0] = float('nan')
    rejected(got, ref, A, ('softmax', 'out'), extra=extra)
