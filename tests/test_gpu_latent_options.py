"""The latent-code options of the reference's loss block on the MI355X: the KL term (lambda_kl), the learned modality prior (is_distri_z)
and mean compaction (s_compact_method 'mean').  The new kernels (csrc/mrdis_latent.hip) element-wise against float64, one training step
per option against vectors from the real reference (tools/gen_golden_kl.py), graph replay, the prior left alone when nothing reads it,
the compute dtypes, the entry point and the nearest-neighbour evaluation."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

from fixtures import make_inputs, reinit_discriminator

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
PAD_C = 3


@pytest.fixture(scope='module')
def mrdis():
    import mrdis as m
    assert torch.cuda.is_available()
    m.hip.load()
    return m


def cl(x):
    return x.to(DEV).contiguous(memory_format=torch.channels_last)


def rnd(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ------------------------------------------------------------------------------------------------ KL vs float64
def _kl_ref(mu, lv, w, pm=None, plv=None):
    """float64 reference: mu, lv (M, B, Z); w (M, B); pm, plv (M, Z) or (M, B, Z) or None"""
    if pm is None:
        kl = 0.5 * (torch.exp(lv) + mu ** 2 - 1 - lv)
    else:
        if pm.dim() == 2:
            pm, plv = pm[:, None], plv[:, None]
        kl = 0.5 * (-1 + (plv - lv) + (torch.exp(lv) + (mu - pm) ** 2) / torch.exp(plv))
    return (kl.sum(2) * w).sum()


KL_CASES = [  # (M, B, Z, prior: None | 'row' | 'sample', absent contrast or None)
    (1, 1, 16, None, None),
    (2, 3, 16, 'row', None),
    (3, 17, 5, 'row', 1),            # contrast 1 absent from every row: its weights are 0, the term gives 0
    (4, 33, 16, None, None),
    (4, 257, 16, 'row', 3),          # more elements than one workgroup's threads
    (2, 5, 7, 'sample', None),       # a per-sample prior (what a caller's own per-row lists become)
]


@pytest.mark.parametrize('case', KL_CASES, ids=lambda c: 'M{}_B{}_Z{}_{}_{}'.format(*c))
def test_kl_vs_float64(mrdis, case):
    M, B, Z, prior, absent = case
    mu, lv = rnd((M, B, Z), 1), rnd((M, B, Z), 2, 0.7)
    mask = (torch.rand(B, M, generator=torch.Generator().manual_seed(3)) > 0.3).float()
    mask[0] = 1.0
    if absent is not None:
        mask[:, absent] = 0.0
    w = torch.zeros(M, B)
    for i in range(M):
        n = float(mask[:, i].sum())
        if n > 0:
            w[i] = mask[:, i] / (M * n)
    w[0, B - 1] = 0.0                                                       # a zero-weight row
    pm = plv = None
    if prior == 'row':
        pm, plv = rnd((M, Z), 4), rnd((M, Z), 5, 0.5)
    elif prior == 'sample':
        pm, plv = rnd((M, B, Z), 4), rnd((M, B, Z), 5, 0.5)
    # strided device blocks: column slices of wider buffers (row stride Z + 3)
    wide_mu = torch.full((M, B, Z + 3), float('nan'), device=DEV)
    wide_lv = torch.full((M, B, Z + 3), float('nan'), device=DEV)
    wide_mu[..., :Z] = mu.to(DEV); wide_lv[..., :Z] = lv.to(DEV)
    mus = [wide_mu[i, :, :Z].detach().requires_grad_(True) for i in range(M)]
    lvs = [wide_lv[i, :, :Z].detach().requires_grad_(True) for i in range(M)]
    assert mus[0].stride(0) == Z + 3
    dp = None if pm is None else (pm.to(DEV).requires_grad_(True), plv.to(DEV).requires_grad_(True))
    mrdis.hip.launch_counts(reset=True)
    loss = mrdis.ops.kl_loss(mus, lvs, w.to(DEV), prior=dp)
    (2.5 * loss).backward()
    assert mrdis.hip.launch_counts()['kl'] == 2                               # one launch each way
    md, lvd = mu.double().requires_grad_(True), lv.double().requires_grad_(True)
    pd = None if pm is None else (pm.double().requires_grad_(True), plv.double().requires_grad_(True))
    ref = _kl_ref(md, lvd, w.double(), *(pd or (None, None)))
    (2.5 * ref).backward()
    assert torch.isfinite(loss) and abs(float(loss.detach()) - float(ref)) <= 1e-5 * abs(float(ref)) + 1e-6, (float(loss.detach()), float(ref))

    def close(got, want, what):
        got = got.detach().double().cpu()
        err = float((got - want).abs().max())
        assert err <= 1e-5 * float(want.abs().max()) + 1e-7, (what, err)
    close(torch.stack([t.grad for t in mus]), md.grad, 'dmu')
    close(torch.stack([t.grad for t in lvs]), lvd.grad, 'dlv')
    if pd is not None:
        close(dp[0].grad, pd[0].grad, 'dpmu'); close(dp[1].grad, pd[1].grad, 'dplv')
    if absent is not None:
        assert float(torch.stack([t.grad for t in mus])[absent].abs().max()) == 0.0
    assert torch.isnan(wide_mu[..., Z:]).all()                                # the padding columns were not written


def test_kl_is_bit_identical_across_launches(mrdis):
    M, B, Z = 4, 96, 16
    mus = [rnd((B, Z), 10 + i).to(DEV) for i in range(M)]
    lvs = [rnd((B, Z), 20 + i, 0.5).to(DEV) for i in range(M)]
    w = torch.full((M, B), 1.0 / (M * B), device=DEV)
    a = mrdis.hip.kl_fwd(mus, lvs, w)
    b = mrdis.hip.kl_fwd(mus, lvs, w)
    assert torch.equal(a, b)


def test_two_gaussian_all_absent_contrast_gives_zero_not_nan(mrdis):
    """the deviation of DESIGN.md section 5: a contrast absent from every row contributes 0 (the reference divides 0 by 0), the division by M stays"""
    cfg = _cfg(mrdis, 3, 64, 64, 4, is_distri_z=True, lambda_kl=1.0)
    torch.manual_seed(1)
    model = mrdis.build_model(cfg)
    B, M, Z = 4, 3, 16
    mus = [rnd((B, Z), i).to(DEV).requires_grad_(True) for i in range(M)]
    lvs = [rnd((B, Z), 5 + i, 0.3).to(DEV).requires_grad_(True) for i in range(M)]
    mask = torch.tensor([[1., 0., 1.], [1., 0., 0.], [0., 0., 1.], [1., 0., 1.]])
    pm, plv = model.compute_zi_prior_distribution(B, M, DEV)
    loss = model.compute_kl_loss_list_two_gaussian(mus, lvs, pm, plv, mask.to(DEV), mask)
    loss.backward()
    assert torch.isfinite(loss)
    # the same sum over the two present contrasts, still divided by M = 3
    with torch.no_grad():
        pmr, plr = model.distri_z(torch.arange(1, M + 1, dtype=torch.float32, device=DEV).view(M, 1))
        want = 0.0
        for i in (0, 2):
            kl = 0.5 * (-1 + (plr[i] - lvs[i]) + (torch.exp(lvs[i]) + (mus[i] - pmr[i]) ** 2) / torch.exp(plr[i]))
            want += float((kl.sum(1) * mask[:, i].to(DEV)).sum() / mask[:, i].sum()) / M
    assert abs(float(loss) - want) <= 1e-5 * abs(want)
    assert float(mus[1].grad.abs().max()) == 0.0
    assert all(torch.isfinite(p.grad).all() for p in model.distri_z.parameters())


# ------------------------------------------------------------------------------------------------ mean pooling vs float64
POOL_CASES = [(2, 4, 37, 50, 16), (3, 4, 256, 256, 16), (1, 5, 20, 33, 4), (2, 4, 16, 16, 16), (2, 3, 47, 31, 16)]


@pytest.mark.parametrize('case', POOL_CASES, ids=lambda c: 'N{}_C{}_{}x{}_k{}'.format(*c))
def test_avg_pool_vs_float64_and_torch(mrdis, case):
    N, C, H, W, k = case
    x = rnd((N, C, H, W), 7)
    wide = torch.cat([rnd((N, PAD_C, H, W), 8), x, rnd((N, PAD_C, H, W), 9)], 1)
    xg = cl(wide)[:, PAD_C:PAD_C + C].requires_grad_(True)                   # a channel slice: pixel stride C + 6
    mrdis.hip.launch_counts(reset=True)
    y = mrdis.ops.avg_pool(xg, k)
    D = C * (H // k) * (W // k)
    assert tuple(y.shape) == (N, D)
    ref = F.avg_pool2d(x.double(), k).reshape(N, -1)
    assert float((y.double().cpu() - ref).abs().max()) <= 1e-6 * float(ref.abs().max()) + 1e-7
    torch_ref = F.avg_pool2d(x.to(DEV), k).reshape(N, -1)
    assert float((y - torch_ref).abs().max()) <= 1e-6
    dy = rnd((N, D), 11)
    y.backward(dy.to(DEV))
    assert mrdis.hip.launch_counts()['avgpool'] == 2
    xd = x.double().requires_grad_(True)
    F.avg_pool2d(xd, k).reshape(N, -1).backward(dy.double())
    g = xg.grad.double().cpu()
    assert float((g - xd.grad).abs().max()) <= 1e-6 * float(xd.grad.abs().max())
    Hf, Wf = k * (H // k), k * (W // k)
    assert float(g[:, :, Hf:].abs().max() if Hf < H else 0.0) == 0.0 and float(g[:, :, :, Wf:].abs().max() if Wf < W else 0.0) == 0.0


# ------------------------------------------------------------------------------------------------ one step vs the real reference
def _cfg(mrdis, M, H, W, B, **kw):
    cfg = dict(mrdis.DEFAULT_CONFIG)
    cfg.update(contrast_list=[f'm{i}' for i in range(M)], input_height=H, input_width=W, batch_size=max(B, 16), **kw)
    return mrdis.derive_config(cfg, DEV)


LATENT_GOLDENS = ['b2m2_kl', 'b2m4_distri_drop', 'b2m2_mean']


def _close(got, want, what, rtol=1e-3):
    got = got.detach().float().cpu()
    want = torch.as_tensor(want).float()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), what
    err = (got - want).abs().max().item()
    assert err <= rtol * float(want.abs().max()) + 1e-7, (what, err, float(want.abs().max()))


@pytest.mark.parametrize('tag', LATENT_GOLDENS)
def test_latent_train_step_golden(mrdis, golden_dir, tag):
    meta = json.load(open(os.path.join(golden_dir, f'step_{tag}.json')))
    arrs = np.load(os.path.join(golden_dir, f'step_{tag}.npz'))
    B, M = meta['B'], meta['M']
    cfg = _cfg(mrdis, M, 160, 192, B, lambda_kl=meta['lambdas']['kl'], is_distri_z=meta['is_distri_z'], s_compact_method=meta['s_compact_method'])
    torch.manual_seed(10); np.random.seed(10)
    model = mrdis.build_model(cfg).train()
    if meta['is_distri_z']:
        reinit_discriminator(model.distri_z, seed=meta['distri_seed'])
    for k, v in meta['wsum_before'].items():
        got = float(model.state_dict()[k].double().sum())
        assert abs(got - v) <= 1e-6 * max(1.0, abs(v)), ('init', k)
    inputs, mask, mask_img = make_inputs(B, M, 160, 192, seed=10, drop=meta['drop'])
    step = mrdis.TrainStep(model, cfg)
    mrdis.hip.launch_counts(reset=True)
    torch.manual_seed(11); np.random.seed(11)
    names = {id(p): n for n, p in model.named_parameters()}
    with mrdis.ops.mix_cache():
        loss, parts, aux = mrdis.forward_losses(model, cfg, cl(inputs), mask.to(DEV), mask_img.to(DEV), mask)
        loss.backward()
    counts = mrdis.hip.launch_counts()
    if meta['lambdas']['kl'] > 0:
        assert counts['kl'] == 2, counts
    if meta['s_compact_method'] == 'mean':
        assert counts['avgpool'] >= 2, counts                                   # sim_s: both compacted maps, forward and backward
    else:
        assert counts['avgpool'] == 0, counts
    assert abs(float(loss) - meta['loss']) <= 1e-3 * abs(meta['loss']), (float(loss), meta['loss'])
    for k, v in meta['parts'].items():
        assert abs(float(parts[k]) - v) <= 1e-3 * abs(v) + 1e-6, (k, float(parts[k]), v)
    _close(torch.stack(aux['mu_list']), arrs['mu'], 'mu'); _close(torch.stack(aux['lv_list']), arrs['lv'], 'lv')
    _close(torch.stack(aux['zi_list']), arrs['z'], 'z')
    _close(F.avg_pool2d(aux['si_list'][0], 8), arrs['s0_pool8'], 's0')
    _close(F.avg_pool2d(aux['xi_fake_list'][0], 8), arrs['xf0_pool8'], 'xf0')
    if 's0_compact' in arrs:
        _close(model.compute_compact_s(aux['si_list'][0]), arrs['s0_compact'], 's0 compact')
    gn = {names[id(p)]: float(p.grad.double().norm()) for p in model.parameters() if p.grad is not None}
    hot = {k: v for k, v in meta['grad_norms'].items() if not k.startswith('output_decoder')}
    assert set(hot) == set(gn)
    total = float(np.sqrt(sum(v * v for v in gn.values())))
    ref_total = float(np.sqrt(sum(v * v for v in hot.values())))
    assert abs(total - ref_total) <= 1e-3 * ref_total, (total, ref_total)
    for k, v in hot.items():
        assert abs(gn[k] - v) <= 1e-3 * (v + 4e-3 * ref_total), (k, gn[k], v)
    if meta['is_distri_z']:
        for k in [k for k in hot if k.startswith('distri_z.')]:                  # the prior's gradients on their own scale
            assert abs(gn[k] - hot[k]) <= 1e-3 * hot[k] + 1e-9, (k, gn[k], hot[k])
    step.optimizer.step(fused_clip=True)
    for k, v in meta['wsum_after'].items():
        if meta['grad_norms'].get(k, 1.0) < 1e-5 * meta['grad_norm']:
            continue
        t = model.state_dict()[k]
        got = float(t.double().sum())
        flips = 2 * cfg['lr'] * np.ceil(1e-3 * t.numel())
        assert abs(got - v) <= 2e-4 * max(1.0, abs(v)) + flips, ('after step', k, got, v)


# ------------------------------------------------------------------------------------------------ graph replay, Adam, compute dtypes
def _batches(mrdis, n, B, M, H, W, drop=True):
    out = []
    for seed in range(40, 400):
        if len(out) == n:
            break
        x, mask, mask_img = mrdis.synthetic_batch(B, M, H, W, seed=seed, drop=drop)
        if mrdis.regular_mask(mask):
            out.append((cl(x), mask, mask_img.to(DEV)))
    assert len(out) == n
    return out


def _run(mrdis, graph, steps, B=8, M=4, H=64, W=96, dtype='f32', **kw):
    cfg = _cfg(mrdis, M, H, W, 16, compute_dtype=dtype, **kw)
    torch.manual_seed(10); np.random.seed(10)
    model = mrdis.build_model(cfg).train()
    step = mrdis.TrainStep(model, cfg)
    if graph:
        step = mrdis.GraphedTrainStep(step)
    data = _batches(mrdis, steps, B, M, H, W)
    torch.manual_seed(100); np.random.seed(100)
    losses = []
    try:
        for x, mask, mask_img in data:
            loss, parts, _ = step(x, mask.to(DEV), mask_img, mask)
            losses.append({k: float(v) for k, v in parts.items()})
        torch.cuda.synchronize()
    finally:
        mrdis.ops.set_compute_dtype('f32')
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu()
    bufs = torch.cat([b.detach().float().reshape(-1) for b in model.buffers()]).cpu()
    return flat, bufs, losses, step, model


GRAPH_OPTS = {'kl': dict(lambda_kl=1.0), 'distri_kl_mean': dict(lambda_kl=1.0, is_distri_z=True, s_compact_method='mean', lambda_adv_s=1.0)}


@pytest.mark.timeout(900)
@pytest.mark.parametrize('name', list(GRAPH_OPTS))
def test_graph_replay_is_bit_identical(mrdis, name):
    """GraphedTrainStep against the eager step over 6 steps whose drop-off masks change every iteration: the KL weights and the prior replay"""
    kw = GRAPH_OPTS[name]
    ref_w, ref_b, ref_l, _, _ = _run(mrdis, False, 6, **kw)
    got_w, got_b, got_l, step, _ = _run(mrdis, True, 6, **kw)
    assert step.stats['replays'] > 0, step.stats
    assert all(l['kl'] > 0 for l in ref_l)
    assert got_l == ref_l
    assert torch.equal(ref_w, got_w), float((ref_w - got_w).abs().max())
    assert torch.equal(ref_b, got_b)


def test_distri_z_untouched_by_adam_without_kl(mrdis):
    """is_distri_z with lambda_kl = 0: nothing reads the prior, so it gets no gradient; like torch's Adam (grad None: skipped) the step leaves
    it bit for bit as it was -- no weight decay, no moments, no checkpoint state -- while the other weights move"""
    cfg = _cfg(mrdis, 2, 64, 64, 4, is_distri_z=True, lambda_kl=0.0)
    torch.manual_seed(10); np.random.seed(10)
    model = mrdis.build_model(cfg).train()
    before = {n: p.detach().clone() for n, p in model.named_parameters() if n.startswith('distri_z.')}
    enc = model.modality_encoder_list[0].mean.weight.detach().clone()
    step = mrdis.TrainStep(model, cfg)
    assert not ({id(p) for p in model.distri_z.parameters()} & step.optimizer.used_ids)
    for x, mask, mask_img in _batches(mrdis, 2, 4, 2, 64, 64, drop=False):   # (M = 2 with drop-off never shares a sample between the contrasts)
        step(x, mask.to(DEV), mask_img, mask)                              # batch_size 16: every call steps
    torch.cuda.synchronize()
    assert float(step.optimizer.step_state[0]) == 2
    for n, p in model.named_parameters():
        if n.startswith('distri_z.'):
            assert torch.equal(p.detach(), before[n]) and p.grad is None, n
    assert not torch.equal(model.modality_encoder_list[0].mean.weight.detach(), enc)
    idx = {id(p): i for i, p in enumerate(model.parameters())}
    sd = step.optimizer.state_dict()
    assert not ({idx[id(p)] for p in model.distri_z.parameters()} & set(sd['state']))


@pytest.mark.parametrize('dtype', ['bf16m', 'bf16'])
def test_compute_dtypes_run_the_latent_options(mrdis, dtype):
    """'bf16m' and 'bf16': the KL reads the fp32 Linear outputs, the compaction the fp32 anatomy maps -- two steps, finite and close to f32"""
    kw = dict(lambda_kl=1.0, is_distri_z=True, s_compact_method='mean')
    w32, _, l32, _, _ = _run(mrdis, False, 2, **kw)
    w16, _, l16, _, _ = _run(mrdis, False, 2, dtype=dtype, **kw)
    assert torch.isfinite(w16).all() and all(np.isfinite(v) for l in l16 for v in l.values())
    for k, v in l32[0].items():
        assert abs(v - l16[0][k]) <= 2e-2 * abs(v) + 1e-4, (k, v, l16[0][k])


# ------------------------------------------------------------------------------------------------ entry point, evaluation
@pytest.mark.timeout(900)
def test_entry_point_trains_resumes_and_evaluates_with_kl(mrdis, tmp_path):
    """config.yaml with lambda_kl, is_distri_z and s_compact_method 'mean': one epoch through train.Run (checkpoint written), a resumed run
    whose optimizer state includes distri_z's moments and steps exactly as the original, and the evaluation reporting kl"""
    m = mrdis
    base = dict(contrast_list=['T1', 'T2'], input_height=64, input_width=64, batch_size=4, epochs=1, gpu='0', data_source='synthetic',
                ckpt_root=str(tmp_path / 'ckpt'), ckpt_timelabel='t0', shuffle=False, lambda_kl=0.5, is_distri_z=True, s_compact_method='mean')
    (tmp_path / 'config.yaml').write_text(yaml.dump(base))
    cfg = m.train.setup_config(str(tmp_path / 'config.yaml'), device=DEV)
    run = m.train.Run(cfg, log=lambda *a: None)
    run.train(max_iters_per_epoch=4)
    d = cfg['ckpt_path']
    ck = torch.load(os.path.join(d, 'epoch000.pth.tar'), weights_only=False)
    assert 'distri_z.linear.2.weight' in ck['model'] and ck['stat']['kl'] > 0
    idx = {id(p): i for i, p in enumerate(run.model.parameters())}
    prior_idx = {idx[id(p)] for p in run.model.distri_z.parameters()}
    assert prior_idx <= set(ck['optimizer']['state'])                      # distri_z was stepped and its moments are saved
    x, mask, mask_img = m.synthetic_batch(4, 2, 64, 64, seed=5)
    args = (cl(x), mask.to(DEV), mask_img.to(DEV), mask)

    def four_more(r):
        if r.step.acc is not None:
            r.step.acc.zero_()
        torch.manual_seed(77); np.random.seed(77)
        for it in range(4):
            r.step(*args, it=it)
        return r.optimizer.flat_p.clone(), r.optimizer.m.clone()
    want_p, want_m = four_more(run)
    cfg2 = m.train.setup_config(str(tmp_path / 'config.yaml'), overrides={'continue_train': True, 'ckpt_name': 'epoch000.pth.tar',
                                                                          'ckpt_timelabel': os.path.basename(d)}, device=DEV)
    run2 = m.train.Run(cfg2, loaders=run.loaders, log=lambda *a: None)
    assert run2.model.is_distri_z and run2.model.s_compact_method == 'mean'
    got_p, got_m = four_more(run2)
    assert torch.equal(want_p, got_p) and torch.equal(want_m, got_m)
    stat = run2.evaluate(phase='test', set_='test', max_batches=2)
    assert stat['kl'] > 0 and np.isfinite(stat['all'])
    # the reference's evaluate() reports kl without adding it to the loss (main_missing.py:474-480)
    parts_sum = sum(stat[k] * cfg[f'lambda_{k}'] for k in ('recon_x', 'recon_x_mix', 'latent_z', 'sim_s', 'sim_z'))
    assert abs(stat['all'] - parts_sum) <= 1e-4 * abs(parts_sum)


@pytest.mark.timeout(900)
def test_nearest_neighbour_evaluation_under_mean_compaction(mrdis, tmp_path, monkeypatch):
    """build_z_gallery and Run.evaluate(info='nearest_neighbour') with s_compact_method 'mean': the gallery is tagged, its codes and the queries
    come from the mean-pooling kernel; a gallery built by a max-compacting model is refused by EvalStep and rebuilt by Run.z_gallery"""
    m = mrdis
    store = m.train.synthetic_store
    monkeypatch.setattr(m.train, 'synthetic_store', lambda config, device: store(config, device, n_subj=10))
    base = dict(contrast_list=['T1', 'T2'], input_height=64, input_width=64, batch_size=4, epochs=1, gpu='0', data_source='synthetic',
                ckpt_root=str(tmp_path / 'ckpt'), ckpt_timelabel='t0', shuffle=False, s_compact_method='mean')
    (tmp_path / 'train.yaml').write_text(yaml.dump(base))
    cfg = m.train.setup_config(str(tmp_path / 'train.yaml'), device=DEV)
    run = m.train.Run(cfg, log=lambda *a: None)
    run.train(max_iters_per_epoch=2)
    m.hip.launch_counts(reset=True)
    gal = m.build_z_gallery(run, run.loaders['test'])
    assert gal.compact_method == 'mean' and m.hip.launch_counts()['avgpool'] > 0
    D = 4 * (64 // 16) * (64 // 16)
    assert gal.s_compact.shape[2] == D
    m.hip.launch_counts(reset=True)
    stat = run.evaluate(phase='test', set_='test', info='nearest_neighbour')
    c = m.hip.launch_counts()
    assert c['zsearch'] >= 2 and c['avgpool'] > 0
    assert {'rmse', 'psnr', 'ssim', 'recon_x_mix', 'all'} <= set(stat) and np.isfinite(stat['all'])
    # a gallery of max-pooled codes (same shape: both pool 16 x 16) must never be searched with mean-pooled queries
    cfg_max = dict(cfg, s_compact_method='max')
    model_max = m.build_model(cfg_max)
    model_max.load_state_dict(run.model.state_dict())
    gal_max = m.build_z_gallery(model_max, run.loaders['test'], cfg_max)
    assert gal_max.compact_method == 'max' and gal_max.s_compact.shape == gal.s_compact.shape
    with pytest.raises(ValueError, match='not comparable'):
        m.EvalStep(run.model, cfg, info='nearest_neighbour', gallery=gal_max)
    gal_max.save(run.z_gallery_path('test'))
    assert run.z_gallery('test').compact_method == 'mean'                  # rebuilt, not searched
