"""The fusion of the anatomy maps over the contrasts a sample has (csrc/mrdis_fuse.hip, ops.fuse_present, lambda_recon_y_fused) on the MI355X:
the two kernels element by element against a float64 restatement written here, the launch counter, the full training step against a torch
composition of the same rule, the identity at M = 1, graph replay with a different mask per step, and EvalStep's metrics of the fused output."""
import os

import numpy as np
import pytest
import torch

from fixtures import make_inputs, make_seg_targets
from fixtures_outdec import make_float_targets

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
METHODS = ('mean', 'max', 'mean-max-min')
U = 2.0 ** -24                       # unit roundoff of fp32
# tests/test_gpu_output_decoders.py compares HIP results with torch (float64) at max|got - want| / max|want| <= 2e-6 for activations, scalars
# and data gradients and <= 5e-5 for parameter gradients: the same two bounds hold between the two runs of a step here.  A parameter whose true
# gradient is zero (a convolution bias in front of a BatchNorm) holds nothing but the rounding noise of its sums, which no bound relative to its
# own maximum can cover; that file's step comparison gives such parameters a floor relative to the step's TOTAL gradient norm, and so does
# this one, at the tighter of the two relative bounds (2e-6 of the total norm).
TOL, TOL_W = 2e-6, 5e-5


def cl(x):
    return x.to(DEV).contiguous(memory_format=torch.channels_last)


# ------------------------------------------------------------------------------------------- kernels against float64
def _maps(K, B, C, H, W, seed):
    """(K, B, C, H, W) float32 softmax-like maps with exact cross-contrast ties on about a quarter of the pixels: all contrasts equal, all 0 (the
    background of the softmax maps), or a pair of contrasts equal and raised to the pixel's maximum"""
    g = np.random.RandomState(seed)
    z = g.randn(K, B, C, H, W)
    e = np.exp(z - z.max(2, keepdims=True))
    s = (e / e.sum(2, keepdims=True)).astype(np.float32)
    kind = g.rand(B, H, W)
    same, zero, pair = kind < 0.09, (kind >= 0.09) & (kind < 0.17), (kind >= 0.17) & (kind < 0.25)
    for b, h, w in zip(*np.nonzero(same)):
        s[:, b, :, h, w] = s[0, b, :, h, w]
    for b, h, w in zip(*np.nonzero(zero)):
        s[:, b, :, h, w] = 0.0
    if K >= 2:
        for b, h, w in zip(*np.nonzero(pair)):
            i, j = g.choice(K, 2, replace=False)
            top = s[:, b, :, h, w].max(0)
            s[i, b, :, h, w] = top
            s[j, b, :, h, w] = top
    return s


def _masks(B, K):
    """all present; exactly one present per row, a different k per row; mixed"""
    one = np.zeros((B, K), dtype=np.float32)
    for b in range(B):
        one[b, (K - 1 - b) % K] = 1
    g = np.random.RandomState(100 + K)
    mixed = (g.rand(B, K) < 0.5).astype(np.float32)
    mixed[0, :] = 1
    mixed[0, K // 2] = 0 if K > 1 else 1
    for b in range(B):
        if mixed[b].sum() == 0:
            mixed[b, b % K] = 1
    return {'all': np.ones((B, K), dtype=np.float32), 'one': one, 'mixed': mixed}


def _ref(s, mask, method, dout):
    """float64 restatement: s (K, B, C, H, W), mask (B, K), dout (B, F C, H, W) -> out, the mean bound's scale, grads (K, B, C, H, W), the sum of
    the absolute gradient terms"""
    K, B, C, H, W = s.shape
    s64, d64 = s.astype(np.float64), dout.astype(np.float64)
    F = 3 if method == 'mean-max-min' else 1
    out = np.zeros((B, F * C, H, W)); scale = np.zeros((B, C, H, W))
    grads = np.zeros(s.shape); terms = np.zeros(s.shape)
    for b in range(B):
        ks = [k for k in range(K) if mask[b, k] == 1]
        n = len(ks)
        tot = np.zeros((C, H, W))
        for k in ks:                                                    # increasing k
            tot = tot + s64[k, b]
        mean = tot / n
        scale[b] = sum(np.abs(s64[k, b]) for k in ks) / n
        stack = s64[ks, b]
        mx, mn = stack.max(0), stack.min(0)
        ax = np.array(ks)[(stack == mx).argmax(0)]                      # argmax of a boolean: the first True = the lowest present index
        an = np.array(ks)[(stack == mn).argmax(0)]
        if method == 'mean':
            out[b] = mean
        elif method == 'max':
            out[b] = mx
        else:
            out[b] = np.concatenate([mean, mx, mn], 0)
        for k in ks:
            if method == 'mean':
                parts = [d64[b] / n]
            elif method == 'max':
                parts = [np.where(ax == k, d64[b], 0.0)]
            else:
                parts = [d64[b, :C] / n, np.where(ax == k, d64[b, C:2 * C], 0.0), np.where(an == k, d64[b, 2 * C:], 0.0)]
            grads[k, b] = sum(parts)
            terms[k, b] = sum(np.abs(p) for p in parts)
    return out, scale, grads, terms


def _view(t, pad, fill=None):
    """t (B, C, H, W) as a channel slice [pad, pad + C) of a channels-last buffer with C + 2 pad channels (pad 0: a dense tensor); fill: the
    buffer is filled with it and t's values are NOT copied (an output view)"""
    B, C, H, W = t.shape
    buf = cl(torch.full((B, C + 2 * pad, H, W), float('nan') if fill is None else fill))
    v = buf[:, pad:pad + C]
    if fill is None:
        v.copy_(t)
    return buf, v


def _outside_untouched(buf, pad, C):
    return pad == 0 or bool(torch.isnan(buf[:, :pad]).all() and torch.isnan(buf[:, pad + C:]).all())


@pytest.mark.parametrize('HW', [(5, 6), (16, 16), (7, 33)], ids=str)
@pytest.mark.parametrize('C', [4, 3, 8])
@pytest.mark.parametrize('K', [1, 2, 3, 4, 8])
def test_fuse_kernels_vs_float64(mrdis, K, C, HW):
    """forward and backward, every method and mask kind, on dense tensors and on channel-slice views with pixel stride > C (inputs and outputs):
    max / min bit-equal both ways (including WHICH index gets the gradient on a tie), the mean within (K + 2) 2^-24 mean_k|s_k|, the mean and
    mean-max-min gradients within 3 * 2^-24 * sum|terms|, an absent contrast's gradient exactly 0, every output element written (NaN pre-fill),
    nothing written outside a view.  C = 3 takes the scalar form; a view at an odd channel offset takes it for C % 4 == 0 too."""
    hip = mrdis.hip
    H, W = HW
    B = 3
    s = _maps(K, B, C, H, W, seed=1000 * K + 10 * C + H)
    pads = [0, 4, 1] if C % 4 == 0 else [0, 1]
    g = np.random.RandomState(7)
    for pad in pads:
        srcs = [_view(torch.from_numpy(s[k]), pad)[1] for k in range(K)]
        for mname, mask in _masks(B, K).items():
            mdev = torch.from_numpy(mask).to(DEV)
            for method in METHODS:
                F = 3 if method == 'mean-max-min' else 1
                dout = g.randn(B, F * C, H, W).astype(np.float32)
                want, scale, wgrads, wterms = _ref(s, mask, method, dout)
                tag = (pad, mname, method)
                obuf, oview = _view(torch.empty(B, F * C, H, W), pad, fill=float('nan'))
                got = hip.fuse_present_fwd(srcs, mdev, method, out=oview)
                assert got.data_ptr() == oview.data_ptr() and _outside_untouched(obuf, pad, F * C), tag
                got = got.cpu().numpy()
                assert not np.isnan(got).any(), tag
                if method == 'max':
                    assert np.array_equal(got, want.astype(np.float32)), tag
                else:
                    assert (np.abs(got[:, :C].astype(np.float64) - want[:, :C]) <= (K + 2) * U * scale).all(), tag
                if method == 'mean-max-min':
                    assert np.array_equal(got[:, C:], want[:, C:].astype(np.float32)), tag
                _, dview = _view(torch.from_numpy(dout), pad)
                gbufs, gviews = zip(*[_view(torch.empty(B, C, H, W), pad, fill=float('nan')) for _ in range(K)])
                grads = hip.fuse_present_bwd(dview, srcs, mdev, method, outs=list(gviews))
                for k in range(K):
                    assert grads[k].data_ptr() == gviews[k].data_ptr() and _outside_untouched(gbufs[k], pad, C), tag
                    gk = grads[k].cpu().numpy()
                    assert not np.isnan(gk).any(), (tag, k)
                    for b in range(B):
                        if mask[b, k] != 1:
                            assert not gk[b].any(), (tag, k, b)                          # exactly 0
                    if method == 'max':
                        assert np.array_equal(gk, wgrads[k].astype(np.float32)), (tag, k)
                    else:
                        assert (np.abs(gk.astype(np.float64) - wgrads[k]) <= 3 * U * wterms[k]).all(), (tag, k)
    # the tie rule of min on its own: with zero gradients for the mean and max parts, mean-max-min's gradient is min's, bit for bit
    mask = _masks(B, K)['mixed']
    dout = g.randn(B, 3 * C, H, W).astype(np.float32)
    dout[:, :2 * C] = 0
    _, _, wgrads, _ = _ref(s, mask, 'mean-max-min', dout)
    srcs = [cl(torch.from_numpy(s[k])) for k in range(K)]
    grads = hip.fuse_present_bwd(cl(torch.from_numpy(dout)), srcs, torch.from_numpy(mask).to(DEV), 'mean-max-min')
    for k in range(K):
        assert np.array_equal(grads[k].cpu().numpy(), wgrads[k].astype(np.float32)), k


def test_fuse_counts_once_per_call_and_a_refused_call_launches_nothing(mrdis):
    hip, ops = mrdis.hip, mrdis.ops
    B, K, C, H, W = 2, 3, 4, 5, 6
    s = _maps(K, B, C, H, W, seed=3)
    srcs = [cl(torch.from_numpy(s[k])) for k in range(K)]
    mask = torch.tensor([[1., 0., 1.], [0., 1., 0.]]).to(DEV)
    torch.cuda.synchronize()

    def delta(fn):
        before = hip.launch_counts(elem=True)
        fn()
        after = hip.launch_counts(elem=True)
        return {k: after[k] - before[k] for k in after if after[k] != before[k]}
    for method in METHODS:
        F = 3 if method == 'mean-max-min' else 1
        assert delta(lambda: hip.fuse_present_fwd(srcs, mask, method)) == {'fuse': 1, 'all': 1}
        dout = cl(torch.ones(B, F * C, H, W))
        assert delta(lambda: hip.fuse_present_bwd(dout, srcs, mask, method)) == {'fuse': 1, 'all': 1}

    def refused(exc, fn):
        def run():
            with pytest.raises(exc):
                fn()
        assert delta(run) == {}
    refused(mrdis.MrdisError, lambda: hip.fuse_present_fwd(srcs * 3, torch.ones(B, 9, device=DEV), 'mean'))
    refused(mrdis.MrdisError, lambda: hip.fuse_present_fwd(srcs, mask, 'median'))
    refused(mrdis.MrdisError, lambda: hip.fuse_present_fwd(srcs, mask[:, :2].contiguous(), 'mean'))
    refused(ValueError, lambda: ops.fuse_present(srcs, mask, np.array([[1, 0, 1], [0, 0, 0]], dtype=np.float32), 'max'))
    refused(ValueError, lambda: ops.fuse_present(srcs, mask, mask.cpu(), 'min'))
    lib = hip.load()
    assert delta(lambda: lib.mrdis_fuse_present_fwd(None, None, 9, None, 0, None, 4, 2, 30, 4, None)) == {}      # the C entry point's own refusal


def test_fuse_autograd_matches_the_kernels(mrdis):
    """ops.fuse_present: the autograd pairing hands the maps' gradients back in order, None for the mask"""
    B, K, C, H, W = 2, 3, 4, 6, 5
    s = _maps(K, B, C, H, W, seed=9)
    mask = np.array([[1, 1, 0], [0, 1, 1]], dtype=np.float32)
    mdev = torch.from_numpy(mask).to(DEV)
    for method in METHODS:
        F = 3 if method == 'mean-max-min' else 1
        srcs = [cl(torch.from_numpy(s[k])).requires_grad_() for k in range(K)]
        out = mrdis.ops.fuse_present(srcs, mdev, mask, method)
        dout = cl(torch.randn(B, F * C, H, W, generator=torch.Generator().manual_seed(1)))
        out.backward(dout)
        want = mrdis.hip.fuse_present_bwd(dout, [t.detach() for t in srcs], mdev, method)
        assert torch.equal(out.detach(), mrdis.hip.fuse_present_fwd([t.detach() for t in srcs], mdev, method))
        for k in range(K):
            assert torch.equal(srcs[k].grad, want[k]), (method, k)


# ------------------------------------------------------------------------------------------- the full step against a torch composition
def torch_fuse(si_list, mask, mask_host, method):
    """the rule of ops.fuse_present as a torch composition: the mean as the sum in increasing k over the count; max / min through amax / amin, the
    gradient routed to the lowest present index that attains the extremum (torch's own amax backward would split it evenly over a tie)"""
    s = torch.stack(si_list, 1)                                             # (B, K, C, H, W)
    pres = (mask == 1)[:, :, None, None, None]
    n = pres.sum(1).float()

    def extremum(sign):
        vals = torch.where(pres, sign * s.detach(), torch.full_like(s, float('-inf')))
        hit = pres & (vals == vals.amax(1, keepdim=True))
        first = hit & (hit.cumsum(1) == 1)
        return (s * first).sum(1)                                           # one value and zeros: exact
    acc = None
    for k in range(len(si_list)):
        term = torch.where(pres[:, k], si_list[k], torch.zeros_like(si_list[k]))
        acc = term if acc is None else acc + term
    mean = acc / n
    if method == 'mean':
        out = mean
    elif method == 'max':
        out = extremum(1.0)
    else:
        out = torch.cat([mean, extremum(1.0), extremum(-1.0)], 1)
    return out.contiguous(memory_format=torch.channels_last)


def _cfg(mrdis, M, method, dataset='BraTS', H=64, W=64, **kw):
    cfg = dict(mrdis.DEFAULT_CONFIG)
    cfg.update(contrast_list=[f'm{i}' for i in range(M)], input_height=H, input_width=W, batch_size=16, lambda_recon_y_fused=1.0,
               fuse_method=method, out_num_ch=4 if dataset == 'BraTS' else 1, dataset_name=dataset)
    if dataset != 'BraTS':
        cfg.update(norm_type='mean')
    cfg.update(kw)
    return mrdis.derive_config(cfg, DEV)


def _batch(B, M, H, W, seed, dropped, dataset='BraTS'):
    """a seeded batch with the contrasts `dropped` = [(b, k), ...] (k >= 1) hidden as the loader hides them: zero channels, mask 0"""
    x, mask, mask_img = make_inputs(B, M, H, W, seed=seed)
    for b, k in dropped:
        assert k >= 1                                                       # mask_img comes from contrast 0
        x[b, 7 * k:7 * (k + 1)] = 0
        mask[b, k] = 0
    tg = make_seg_targets(B, H, W, seed=seed + 1) if dataset == 'BraTS' else make_float_targets(B, H, W, seed=seed + 1)
    return cl(x), mask.to(DEV), mask_img.to(DEV), mask, tg.to(DEV)


def _rel(got, want):
    got, want = got.double(), want.double()
    return float((got - want).abs().max()) / (float(want.abs().max()) + 1e-30)


@pytest.mark.parametrize('M,method,dataset', [(2, 'mean', 'BraTS'), (3, 'max', 'BraTS'), (3, 'mean-max-min', 'BraTS'), (2, 'max', 'PET')],
                         ids=lambda v: str(v))
def test_full_step_matches_the_torch_composition(mrdis, monkeypatch, M, method, dataset):
    """B 2, 64 x 64 (at 32 x 32 the decoders' instance norms see one pixel), lambda_recon_y_fused = 1, a drop-off row: forward, every loss part
    and every parameter gradient with ops.fuse_present and with the torch composition in its place, same model, same seeds"""
    B, H, W = 2, 64, 64
    cfg = _cfg(mrdis, M, method, dataset)
    torch.manual_seed(10); np.random.seed(10)
    model = mrdis.build_model(cfg).train()
    x, mask, mask_img, mask_host, tg = _batch(B, M, H, W, seed=21, dropped=[(1, M - 1)], dataset=dataset)

    def run():
        model.zero_grad(set_to_none=True)
        torch.manual_seed(11); np.random.seed(11)
        with mrdis.ops.mix_cache():
            loss, parts, aux = mrdis.forward_losses(model, cfg, x, mask, mask_img, mask_host, targets=tg)
            loss.backward()
        return ({k: v.detach().clone() for k, v in parts.items()}, aux['y_fused'].detach().clone(),
                {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})
    before = mrdis.hip.launch_counts()['fuse']
    parts_h, y_h, grads_h = run()
    assert mrdis.hip.launch_counts()['fuse'] == before + 2
    monkeypatch.setattr(mrdis.ops, 'fuse_present', torch_fuse)
    parts_t, y_t, grads_t = run()
    assert mrdis.hip.launch_counts()['fuse'] == before + 2
    assert float(parts_h['recon_y_fused']) > 0 and float(parts_h['recon_y']) == 0
    assert y_h.shape[0] == B
    assert _rel(y_h, y_t) <= TOL
    for k in parts_h:
        assert _rel(parts_h[k], parts_t[k]) <= TOL, (k, float(parts_h[k]), float(parts_t[k]))
    assert set(grads_h) == set(grads_t) and any(n.startswith('output_decoder.') for n in grads_h)
    total = float(torch.sqrt(sum(g.double().pow(2).sum() for g in grads_t.values())))
    for n in grads_h:
        diff, top = float((grads_h[n].double() - grads_t[n].double()).abs().max()), float(grads_t[n].abs().max())
        assert diff <= TOL_W * top + TOL * total, (n, diff, top, total)


@pytest.mark.parametrize('method', METHODS)
def test_one_contrast_fused_equals_the_per_contrast_term(mrdis, method):
    """M = 1: the fusion is the identity, so with equal lambdas recon_y_fused is recon_y bit for bit (the terms that need two contrasts are off)"""
    B, H, W = 2, 64, 64
    cfg = _cfg(mrdis, 1, method, lambda_recon_y=1.0, lambda_sim_s=0.0, lambda_sim_z=0.0, lambda_recon_x_mix=0.0)
    torch.manual_seed(10); np.random.seed(10)
    model = mrdis.build_model(cfg).train()
    x, mask, mask_img, mask_host, tg = _batch(B, 1, H, W, seed=31, dropped=[])
    torch.manual_seed(11); np.random.seed(11)
    with mrdis.ops.mix_cache():
        loss, parts, aux = mrdis.forward_losses(model, cfg, x, mask, mask_img, mask_host, targets=tg)
        loss.backward()
    assert float(parts['recon_y']) > 0
    assert torch.equal(parts['recon_y_fused'], parts['recon_y'])
    assert torch.equal(aux['y_fused'], aux['y_list'][0])


GRAPH_MASKS = [[[1, 1], [1, 1], [1, 1], [1, 1]], [[1, 1], [1, 1], [1, 1], [1, 1]],           # the two eager warm-up steps
               [[1, 1], [1, 1], [1, 0], [0, 1]], [[1, 0], [1, 1], [0, 1], [1, 1]], [[1, 1], [0, 1], [1, 1], [1, 0]]]      # the three replayed ones


def test_graph_replay_with_a_different_mask_per_step_is_bit_identical(mrdis):
    """the kernels read the mask on the device, so ONE recording serves every mask: three replayed steps, each with its own drop-off pattern,
    equal the same steps run eagerly bit for bit (losses, loss parts and weights)"""
    B, M, H, W = 4, 2, 64, 64
    res = {}
    for graph in (False, True):
        cfg = _cfg(mrdis, M, 'mean-max-min')
        torch.manual_seed(10); np.random.seed(10)
        model = mrdis.build_model(cfg).train()
        step = mrdis.TrainStep(model, cfg)
        if graph:
            step = mrdis.GraphedTrainStep(step)
        torch.manual_seed(100); np.random.seed(100)
        seen = []
        for it, rows in enumerate(GRAPH_MASKS):
            mh = np.array(rows, dtype=np.float32)
            assert mrdis.regular_mask(mh)
            dropped = [(b, k) for b in range(B) for k in range(M) if mh[b, k] == 0 and k >= 1]
            x, mask, mask_img, _, tg = _batch(B, M, H, W, seed=40 + it, dropped=dropped)
            mask = torch.from_numpy(mh).to(DEV)                              # (a hidden contrast 0 keeps its channels: only the mask matters here)
            loss, parts, _ = step(x, mask, mask_img, torch.from_numpy(mh), targets=tg)
            seen.append((float(loss), float(parts['recon_y_fused'])))
        torch.cuda.synchronize()
        if graph:
            assert step.stats['replays'] == 3 and step.stats['captures'] == 1, step.stats
        res[graph] = (seen, torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu())
    assert res[True][0] == res[False][0]
    assert len({v for _, v in res[True][0][2:]}) == 3                        # the masks did change the fused term
    assert torch.equal(res[True][1], res[False][1])


def test_graph_replay_refuses_a_sample_without_a_present_contrast(mrdis):
    """(host only) the check the eager step makes inside ops.fuse_present, which a replay would skip"""
    with pytest.raises(ValueError):
        mrdis.ops.check_fuse_mask(np.array([[1, 1], [0, 0]], dtype=np.float32))


def test_bf16m_runs_the_fused_term(mrdis):
    cfg = _cfg(mrdis, 2, 'mean', compute_dtype='bf16m')
    try:
        torch.manual_seed(10); np.random.seed(10)
        model = mrdis.build_model(cfg).train()
        step = mrdis.TrainStep(model, cfg)
        x, mask, mask_img, mask_host, tg = _batch(2, 2, 64, 64, seed=3, dropped=[(0, 1)])
        before = mrdis.hip.launch_counts()['fuse']
        loss, parts, _ = step(x, mask, mask_img, mask_host, targets=tg)
        assert np.isfinite(float(loss)) and float(parts['recon_y_fused']) > 0
        assert mrdis.hip.launch_counts()['fuse'] == before + 2
    finally:
        mrdis.ops.set_compute_dtype('f32')


# ------------------------------------------------------------------------------------------- evaluation
@pytest.fixture(scope='module')
def eval_setup(mrdis):
    B, M, H, W = 2, 3, 64, 64
    cfg = _cfg(mrdis, M, 'mean-max-min')
    torch.manual_seed(10); np.random.seed(10)
    model = mrdis.build_model(cfg)
    batch = _batch(B, M, H, W, seed=51, dropped=[(1, 2)])
    # a freshly initialised decoder's raw output stays far below the metrics' 0.5 threshold: move the last convolution's bias (the output is
    # linear in it) so that each scored channel's median sits ON the threshold and the thresholded maps are neither empty nor full
    x, mask, mask_img, mask_host, tg = batch
    y = mrdis.EvalStep(model, cfg)(x, mask, mask_img, mask_host, targets=tg)[3]['y_fused'].float()
    with torch.no_grad():
        model.output_decoder.output.up[1].bias[:3] += 0.5 - y[:, :3].transpose(0, 1).reshape(3, -1).median(1).values
    return model, cfg, batch


def _np_segmentation_metrics(target, pred):
    """util.py:980-992 restated: per sample, output channel i thresholded at 0.5 against label i + 1"""
    dice, iou = [], []
    for b in range(target.shape[0]):
        t = target[b, 0]
        d, u = [], []
        for i in range(3):
            a, p = t == i + 1, pred[b, i] > 0.5
            inter, union = np.logical_and(a, p), np.logical_or(a, p)
            d.append((2. * inter.sum() + 1) / (a.sum() + p.sum() + 1))
            u.append((np.sum(inter) + 1) / (np.sum(union) + 1))
        dice.append(np.mean(d)); iou.append(np.mean(u))
    return np.array(dice), np.array(iou)


def test_eval_step_scores_the_fused_output(mrdis, eval_setup):
    model, cfg, (x, mask, mask_img, mask_host, tg) = eval_setup
    torch.manual_seed(11); np.random.seed(11)
    loss, parts, metrics, aux = mrdis.EvalStep(model, cfg)(x, mask, mask_img, mask_host, targets=tg)
    assert set(metrics) == {'dice', 'iou'} and metrics['dice'].shape == (x.shape[0],)
    assert float(parts['recon_y_fused']) > 0 and model.training          # (EvalStep puts the mode back)
    dice, iou = _np_segmentation_metrics(tg.cpu().numpy(), aux['y_fused'].float().cpu().numpy())
    np.testing.assert_allclose(metrics['dice'].cpu().numpy(), dice, rtol=1e-14, atol=0)
    np.testing.assert_allclose(metrics['iou'].cpu().numpy(), iou, rtol=1e-14, atol=0)
    y = aux['y_fused'].float().cpu().numpy()
    assert 0 < (y[:, :3] > 0.5).mean() < 1                                  # the thresholded maps are neither empty nor full: the counts are exercised


def test_eval_step_other_datasets_score_the_fused_output_as_an_image(mrdis):
    B, M, H, W = 2, 2, 64, 64
    cfg = _cfg(mrdis, M, 'mean', dataset='PET')
    torch.manual_seed(10); np.random.seed(10)
    model = mrdis.build_model(cfg)
    x, mask, mask_img, mask_host, tg = _batch(B, M, H, W, seed=52, dropped=[(0, 1)], dataset='PET')
    torch.manual_seed(11); np.random.seed(11)
    _, parts, metrics, aux = mrdis.EvalStep(model, cfg)(x, mask, mask_img, mask_host, targets=tg)
    assert set(metrics) == {'rmse', 'psnr', 'ssim'} and metrics['rmse'].shape == (B,)
    want = mrdis.hip.recon_metrics(tg, aux['y_fused'])
    for j, k in enumerate(('rmse', 'psnr', 'ssim')):
        assert torch.equal(metrics[k], want[:, j])


def test_eval_drop_equals_inputs_and_mask_edited_by_hand(mrdis, eval_setup):
    model, cfg, (x, mask, mask_img, mask_host, tg) = eval_setup
    name, j, c = 'm1', 1, 7
    torch.manual_seed(11); np.random.seed(11)
    got = mrdis.EvalStep(model, dict(cfg, eval_drop=[name]))(x, mask, mask_img, mask_host, targets=tg)
    x2, mask2, mh2 = x.clone(), mask.clone(), mask_host.clone()
    x2[:, j * c:(j + 1) * c] = 0
    mask2[:, j] = 0
    mh2[:, j] = 0
    torch.manual_seed(11); np.random.seed(11)
    want = mrdis.EvalStep(model, cfg)(x2, mask2, mask_img, mh2, targets=tg)
    assert torch.equal(got[0], want[0])
    for k in want[1]:
        assert torch.equal(got[1][k], want[1][k]), k
    for k in want[2]:
        assert torch.equal(got[2][k], want[2][k]), k
    assert torch.equal(got[3]['y_fused'], want[3]['y_fused'])
    torch.manual_seed(11); np.random.seed(11)
    plain = mrdis.EvalStep(model, cfg)(x, mask, mask_img, mask_host, targets=tg)
    assert not torch.equal(plain[3]['y_fused'], got[3]['y_fused'])          # hiding the contrast did change the fused output
    assert float(x[:, j * c:(j + 1) * c].abs().sum()) > 0                   # and the caller's batch was left alone


def test_eval_step_without_the_fused_term_is_bit_identical_to_the_parent(mrdis, golden_dir):
    """lambda_recon_y_fused == 0: loss, loss parts and metrics of a seeded batch equal, bit for bit, what the commit before this feature returned
    (tests/golden/eval_nofuse_b2m2.npz, recorded by running that commit's EvalStep with these very lines)"""
    want = np.load(os.path.join(golden_dir, 'eval_nofuse_b2m2.npz'))
    B, M, H, W = 2, 2, 64, 64
    cfg = dict(mrdis.DEFAULT_CONFIG)
    cfg.update(contrast_list=['m0', 'm1'], input_height=H, input_width=W, batch_size=16)
    cfg = mrdis.derive_config(cfg, DEV)
    torch.manual_seed(10); np.random.seed(10)
    model = mrdis.build_model(cfg)
    x, mask, mask_img = make_inputs(B, M, H, W, seed=12, drop=True)
    torch.manual_seed(11); np.random.seed(11)
    loss, parts, metrics, aux = mrdis.EvalStep(model, cfg)(cl(x), mask.to(DEV), mask_img.to(DEV), mask)
    assert set(metrics) == {'rmse', 'psnr', 'ssim'}
    assert np.array_equal(np.float32(float(loss)).view(np.uint32), want['loss'].view(np.uint32))
    got_parts = np.array([float(parts[k]) for k in mrdis.LOSS_KEYS], dtype=np.float32)
    assert np.array_equal(got_parts.view(np.uint32), want['parts'].view(np.uint32)), (got_parts, want['parts'])
    for k in ('rmse', 'psnr', 'ssim'):
        assert np.array_equal(metrics[k].cpu().numpy().view(np.uint32), want[k].view(np.uint32)), k
    assert 'y_fused' in aux and aux['y_fused'] is None
