"""The fully shared input decoder (config.yaml `shared_inp_dec: True`, SPADENew, model.py:2490-2538) on the MI355X: one training step per
fixture against vectors from the real reference (tools/gen_golden_shared_dec.py) on the batched-per-label path and on the per-call path
(MRDIS_GROUPED=0), graph replay, two data-parallel ranks with divergent masks, proof that every convolution runs on library kernels,
the bf16 compute modes and the entry point."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F
import yaml

from fixtures import make_inputs, reinit_discriminator
from fixtures_outdec import make_float_targets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device('cuda:0')
SHIPPED = {'mod_enc_s': False, 'ana_dec_act': 'softmax', 'old': False, 'softmax_remove_mask': True}
ENCS_SOFTPLUS = {'mod_enc_s': True, 'ana_dec_act': 'softplus', 'old': False}


@pytest.fixture(scope='module')
def mrdis():
    import mrdis as m
    assert torch.cuda.is_available()
    m.hip.load()
    return m


@pytest.fixture
def grouped(mrdis, request):
    """the decode path under test: True = the default (one call per label at batch M B), False = MRDIS_GROUPED=0 (one call per pair)"""
    prev = mrdis.ops._GROUPED
    mrdis.ops.set_grouped(request.param)
    yield request.param
    mrdis.ops.set_grouped(prev)


def cl(x):
    return x.to(DEV).contiguous(memory_format=torch.channels_last)


def _cfg(mrdis, M, H, W, B, others, **kw):
    cfg = dict(mrdis.DEFAULT_CONFIG)
    cfg.update(contrast_list=[f'm{i}' for i in range(M)], input_height=H, input_width=W, batch_size=max(B, 16), others=dict(others),
               shared_inp_dec=True, **kw)
    return mrdis.derive_config(cfg, DEV)


def _close(got, want, what, rtol=1e-3):
    got = got.detach().float().cpu()
    want = torch.as_tensor(want).float()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), what
    err = (got - want).abs().max().item()
    assert err <= rtol * float(want.abs().max()) + 1e-7, (what, err, float(want.abs().max()))


# ------------------------------------------------------------------------------------------------ one step vs the real reference
# (tag, others, per-tensor bar a): test_gpu_variants' 1e-3; with the discriminator, test_gpu_model's b2m2_adv bar (its BatchNorm over a batch of
# two 5x6 maps amplifies fp32 rounding)
GOLDENS = [('b2m2_shdec', SHIPPED, 1e-3), ('b2m4_shdec_drop', SHIPPED, 5e-3), ('b2m2_encs_softplus_shdec', ENCS_SOFTPLUS, 1e-3)]


@pytest.mark.timeout(600)
@pytest.mark.parametrize('grouped', [True, False], ids=['batched', 'per_call'], indirect=True)
@pytest.mark.parametrize('tag,others,a', GOLDENS, ids=[t for t, _, _ in GOLDENS])
def test_shared_decoder_train_step_golden(mrdis, golden_dir, grouped, tag, others, a):
    meta = json.load(open(os.path.join(golden_dir, f'step_{tag}.json')))
    arrs = np.load(os.path.join(golden_dir, f'step_{tag}.npz'))
    B, M, adv = meta['B'], meta['M'], meta['adv']
    cfg = _cfg(mrdis, M, 160, 192, B, others, lambda_adv_s=1.0 if adv else 0.0)
    torch.manual_seed(10); np.random.seed(10)
    model = mrdis.build_model(cfg).train()
    assert len(model.input_decoder_list) == 1
    if adv:
        reinit_discriminator(model.discrim_s)
    for k, v in meta['wsum_before'].items():
        got = float(model.state_dict()[k].double().sum())
        assert abs(got - v) <= 1e-6 * max(1.0, abs(v)), ('init', k)
    inputs, mask, mask_img = make_inputs(B, M, 160, 192, seed=10, drop=meta['drop'])
    step = mrdis.TrainStep(model, cfg)
    calls = []
    dec = model.input_decoder_list[0]
    orig = dec.forward
    dec.forward = lambda si, zi, t=None: (calls.append(si.shape[0]), orig(si, zi, t))[1]
    torch.manual_seed(11); np.random.seed(11)
    names = {id(p): n for n, p in model.named_parameters()}
    with mrdis.ops.mix_cache():
        loss, parts, aux = mrdis.forward_losses(model, cfg, cl(inputs), mask.to(DEV), mask_img.to(DEV), mask)
        loss.backward(retain_graph=adv)
    # the decode: M calls at batch M B (batched) or M + M (M - 1) calls at batch B (per call)
    assert calls == ([M * B] * M if grouped else [B] * (M * M)), calls
    assert abs(float(loss) - meta['loss']) <= 1e-3 * abs(meta['loss']), (float(loss), meta['loss'])
    for k, v in meta['parts'].items():
        assert abs(float(parts[k]) - v) <= 1e-3 * abs(v) + 1e-6, (k, float(parts[k]), v)
    _close(torch.stack(aux['mu_list']), arrs['mu'], 'mu'); _close(torch.stack(aux['zi_list']), arrs['z'], 'z')
    _close(F.avg_pool2d(aux['si_list'][0], 8), arrs['s0_pool8'], 's0')
    _close(F.avg_pool2d(aux['xi_fake_list'][0], 8), arrs['xf0_pool8'], 'xf0')
    _close(F.avg_pool2d(aux['xi_fake_mix_list'][0], 8), arrs['xmix0_pool8'], 'xmix0')
    gn = {names[id(p)]: float(p.grad.double().norm()) for p in model.parameters() if p.grad is not None}
    hot = {k: v for k, v in meta['grad_norms'].items() if not k.startswith('output_decoder')}
    assert set(hot) == set(gn)
    total = float(np.sqrt(sum(v * v for v in gn.values())))
    ref_total = float(np.sqrt(sum(v * v for v in hot.values())))
    assert abs(total - ref_total) <= 1e-3 * ref_total, (total, ref_total)
    worst = max((abs(gn[k] - v) / (v + 4e-3 * ref_total), k) for k, v in hot.items())
    print(f'{tag} grouped={grouped}: worst per-tensor gradient-norm deviation {worst[0]:.2e} ({worst[1]})')
    for k, v in hot.items():
        assert abs(gn[k] - v) <= a * (v + 4e-3 * ref_total), (k, gn[k], v)
    step.optimizer.step(fused_clip=True)
    for k, v in meta['wsum_after'].items():
        if meta['grad_norms'].get(k, 1.0) < 1e-5 * meta['grad_norm']:
            continue
        t = model.state_dict()[k]
        got = float(t.double().sum())
        flips = 2 * cfg['lr'] * np.ceil(1e-3 * t.numel())
        assert abs(got - v) <= 2e-4 * max(1.0, abs(v)) + flips, ('after step', k, got, v)


# ------------------------------------------------------------------------------------------------ both decode paths, library kernels only
def _one_step(mrdis, grouped_on, B=4, M=3, H=64, W=96):
    prev = mrdis.ops._GROUPED
    mrdis.ops.set_grouped(grouped_on)
    try:
        cfg = _cfg(mrdis, M, H, W, B, SHIPPED, lambda_adv_s=1.0, lambda_kl=0.5, is_distri_z=True)
        torch.manual_seed(10); np.random.seed(10)
        model = mrdis.build_model(cfg).train()
        step = mrdis.TrainStep(model, cfg)
        x, mask, mask_img = mrdis.synthetic_batch(B, M, H, W, seed=5, drop=True)
        torch.manual_seed(11); np.random.seed(11)
        with mrdis.ops.mix_cache():
            loss, parts, _ = mrdis.forward_losses(model, cfg, cl(x), mask.to(DEV), mask_img.to(DEV), mask)
            loss.backward()
        torch.cuda.synchronize()
        del step
        return float(loss), {k: float(v) for k, v in parts.items()}, {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters()
                                                                      if p.grad is not None}
    finally:
        mrdis.ops.set_grouped(prev)


@pytest.mark.timeout(600)
def test_batched_and_per_call_decodes_agree(mrdis):
    """the default decode (M calls at batch M B) and MRDIS_GROUPED=0 (the reference's M^2 calls at batch B): the same step within fp32
    reordering -- drop-off mask, discriminator, learned prior and KL term composed in"""
    l1, p1, g1 = _one_step(mrdis, True)
    l0, p0, g0 = _one_step(mrdis, False)
    assert abs(l1 - l0) <= 1e-5 * abs(l0), (l1, l0)
    for k in p0:
        assert abs(p1[k] - p0[k]) <= 1e-5 * abs(p0[k]) + 1e-7, (k, p1[k], p0[k])
    assert set(g1) == set(g0) and any(k.startswith('input_decoder_list.0.') for k in g0)
    total = float(torch.sqrt(sum((g.double() ** 2).sum() for g in g0.values())))
    for k in g0:
        err = float((g1[k] - g0[k]).abs().max())
        assert err <= 1e-4 * float(g0[k].abs().max()) + 1e-6 * total, (k, err, float(g0[k].abs().max()))


@pytest.mark.timeout(600)
def test_no_aten_convolution_or_norm_in_a_full_step(mrdis, monkeypatch):
    """F.conv2d and ATen's norms raise during a full step (forward, losses, backward, Adam); the library's launch counter sees the decoder's
    convolutions: the 3x3 SPADE layers on the Winograd kernels, and more launches than the same step without the decoder's calls"""
    def boom(*a, **k):
        raise AssertionError('an ATen convolution / norm ran')
    for name in ('conv2d', 'instance_norm', 'batch_norm', 'group_norm', 'layer_norm'):
        monkeypatch.setattr(F, name, boom)
    monkeypatch.setattr(torch, 'conv2d', boom)
    B, M, H, W = 4, 2, 64, 96
    cfg = _cfg(mrdis, M, H, W, B, SHIPPED, lambda_adv_s=1.0)
    torch.manual_seed(10); np.random.seed(10)
    model = mrdis.build_model(cfg).train()
    step = mrdis.TrainStep(model, cfg)
    x, mask, mask_img = mrdis.synthetic_batch(B, M, H, W, seed=5)
    dec = model.input_decoder_list[0]
    counts = {}
    orig = dec.forward

    def counted(si, zi, t=None):
        before = mrdis.hip.launch_counts()
        y = orig(si, zi, t)
        after = mrdis.hip.launch_counts()
        for k in after:
            counts[k] = counts.get(k, 0) + after[k] - before[k]
        return y
    dec.forward = counted
    loss, _, _ = step(cl(x), mask.to(DEV), mask_img.to(DEV), mask)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss))
    # 6 SPADE blocks x (si_layers + fused gamma|beta + out) + the 1x1 head, M calls: every launch is the library's
    assert counts['all'] >= M * (6 * 3 + 1), counts
    wino = sum(counts[f] for f in mrdis.hip.WINO_FAMILIES if f not in ('all', 'zsearch'))
    assert wino > 0, counts


# ------------------------------------------------------------------------------------------------ graph replay, bf16 modes
def _batches(mrdis, n, B, M, H, W):
    out = []
    for seed in range(40, 400):
        if len(out) == n:
            break
        x, mask, mask_img = mrdis.synthetic_batch(B, M, H, W, seed=seed, drop=True)
        if mrdis.regular_mask(mask):
            out.append((cl(x), mask, mask_img.to(DEV)))
    assert len(out) == n
    return out


def _run(mrdis, graph, steps, others=SHIPPED, B=8, M=4, H=64, W=96, dtype='f32', **kw):
    cfg = _cfg(mrdis, M, H, W, 16, others, lambda_adv_s=1.0, compute_dtype=dtype, **kw)
    torch.manual_seed(10); np.random.seed(10)
    model = mrdis.build_model(cfg).train()
    step = mrdis.TrainStep(model, cfg)
    if graph:
        step = mrdis.GraphedTrainStep(step)
    data = _batches(mrdis, steps, B, M, H, W)
    targets = make_float_targets(B, H, W, seed=13).to(DEV) if cfg['lambda_recon_y'] > 0 else None
    torch.manual_seed(100); np.random.seed(100)
    losses = []
    try:
        for x, mask, mask_img in data:
            loss, parts, _ = step(x, mask.to(DEV), mask_img, mask, targets=targets)
            losses.append({k: float(v) for k, v in parts.items()})
        torch.cuda.synchronize()
    finally:
        mrdis.ops.set_compute_dtype('f32')
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu()
    bufs = torch.cat([b.detach().float().reshape(-1) for b in model.buffers()]).cpu()
    return flat, bufs, losses, step


@pytest.mark.timeout(900)
def test_graph_replay_is_bit_identical_with_the_shared_decoder(mrdis):
    """GraphedTrainStep against the eager step over 8 steps whose drop-off masks change every iteration: mod_enc_s + softplus anatomy maps,
    non-BraTS data (softplus input decoder and the 'U+SSA+CA' output decoder against float targets), discriminator"""
    kw = dict(others=ENCS_SOFTPLUS, lambda_recon_y=1.0, target_model_name='U+SSA+CA', dataset_name='PET', norm_type='mean')
    ref_w, ref_b, ref_l, _ = _run(mrdis, False, 8, **kw)
    got_w, got_b, got_l, step = _run(mrdis, True, 8, **kw)
    assert step.stats['replays'] > 0, step.stats
    assert got_l == ref_l
    assert torch.equal(ref_w, got_w), float((ref_w - got_w).abs().max())
    assert torch.equal(ref_b, got_b)


@pytest.mark.timeout(600)
def test_bf16m_compute_runs_the_shared_decoder(mrdis):
    w32, _, l32, _ = _run(mrdis, False, 2)
    w16, _, l16, _ = _run(mrdis, False, 2, dtype='bf16m')
    assert torch.isfinite(w16).all() and all(np.isfinite(v) for l in l16 for v in l.values())
    for k, v in l32[0].items():
        assert abs(v - l16[0][k]) <= 2e-2 * abs(v) + 1e-4, (k, v, l16[0][k])


def test_bf16_storage_names_the_setting(mrdis):
    cfg = _cfg(mrdis, 2, 64, 64, 4, SHIPPED, compute_dtype='bf16')
    try:
        with pytest.raises(NotImplementedError, match='shared_inp_dec'):
            mrdis.build_model(cfg)
    finally:
        mrdis.ops.set_compute_dtype('f32')


# ------------------------------------------------------------------------------------------------ two data-parallel ranks
DB, DM, DH, DW, DITERS = 4, 3, 64, 96, 4


def _free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close(); return p


def _ddp_batch(mrdis, rank, it, dev):
    x, mask, mask_img = mrdis.synthetic_batch(DB, DM, DH, DW, seed=50 + 10 * it + rank, drop=False)
    if rank == 0:                                        # modality 2 absent from rank 0's whole batch
        mask[:, 2] = 0
        x[:, 7 * 2:7 * 3] = 0
    return x.to(dev).contiguous(memory_format=torch.channels_last), mask, mask_img.to(dev)


def _ddp_build(mrdis, dev):
    cfg = _cfg(mrdis, DM, DH, DW, 8, SHIPPED, lambda_adv_s=1.0)
    cfg['batch_size'] = 8
    torch.manual_seed(10); np.random.seed(10)
    model = mrdis.build_model(cfg).train()
    return model, mrdis.TrainStep(model, cfg, ddp_buckets=4)


def _signature(model, step):
    import hashlib
    opt = step.optimizer
    out = []
    for t in (torch.cat([p.detach().reshape(-1) for p in model.parameters()]), opt.m, opt.v, opt.vmax, step.optimizer_d_s.m, step.optimizer_d_s.v):
        a = t.detach().cpu().contiguous().numpy()
        out.append((hashlib.sha256(a.tobytes()).hexdigest(), float(np.abs(a.astype(np.float64)).sum())))
    return out


def _ddp_worker(rank, world, port, q):
    import datetime
    import traceback
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    try:
        import mrdis
        dev = torch.device('cuda:0')
        torch.cuda.set_device(dev)
        mrdis.hip.load()
        dist.init_process_group('gloo', rank=rank, world_size=world, timeout=datetime.timedelta(seconds=180))
        model, step = _ddp_build(mrdis, dev)
        red = step.reducer
        assert red is not None and red.world == world and red.exchanging and step.optimizer.n_flags == 0
        torch.manual_seed(100 + rank); np.random.seed(100)
        losses = []
        for it in range(DITERS):
            x, mask, mask_img = _ddp_batch(mrdis, rank, it, dev)
            loss, _, _ = step(x, mask.to(dev), mask_img, mask)
            losses.append(float(loss))
        torch.cuda.synchronize()
        q.put((rank, 'ok', _signature(model, step), losses, red.exposed_ms()))
    except BaseException:                                            # noqa: BLE001 -- report instead of leaving the other rank in a collective
        q.put((rank, 'error', traceback.format_exc(), None, None))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def _ddp_emulate(mrdis, dev):
    """one process, both ranks' batches: gradients added (as the sum all-reduce does), the step applied with scale 1 / 2"""
    model, step = _ddp_build(mrdis, dev)
    assert step.reducer is None and step.accum == 2
    states = []
    for r in range(2):
        torch.manual_seed(100 + r); np.random.seed(100)
        states.append((torch.get_rng_state(), np.random.get_state()))
    opt, od = step.optimizer, step.optimizer_d_s
    for it in range(DITERS):
        do_step = step._advance(None)
        kept = []
        for r in range(2):
            torch.set_rng_state(states[r][0]); np.random.set_state(states[r][1])
            x, mask, mask_img = _ddp_batch(mrdis, r, it, dev)
            step._forward_backward(x, mask.to(dev), mask_img, mask, None, do_step, exchange=False)
            states[r] = (torch.get_rng_state(), np.random.get_state())
            kept.append((opt._g_full.clone(), od._g_full.clone()))
            opt._g_full.zero_(); od._g_full.zero_()
        opt._g_full.copy_(kept[0][0] + kept[1][0]); od._g_full.copy_(kept[0][1] + kept[1][1])
        step._apply(0.5, do_step)
    torch.cuda.synchronize()
    return _signature(model, step)


@pytest.mark.timeout(900)
def test_two_ranks_with_divergent_masks_equal_the_summed_gradient_oracle(mrdis):
    """two gloo ranks on the one GPU, rank 0's whole batch without modality 2: the shared decoder's gradient bucket is exchanged on both
    ranks, and both end bit-identical to each other and to the single-process sum of both ranks' gradients"""
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ddp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=400) for _ in range(2)), key=lambda t: t[0])
    for p in procs:
        p.join(60)
    for r in res:
        assert r[1] == 'ok', r[2]
    assert all(p.exitcode == 0 for p in procs)
    (_, _, sig0, losses0, ex0), (_, _, sig1, losses1, ex1) = res
    emu = _ddp_emulate(mrdis, DEV)
    names = ['weights', 'adam m', 'adam v', 'adam vmax', 'adam_d m', 'adam_d v']
    for n, a, b in zip(names, sig0, sig1):
        assert a == b, (n, 'differs across ranks', a, b)
    for n, a, e in zip(names, sig0, emu):
        assert a == e, (n, 'differs from the summed-gradient oracle', a, e)
    assert losses0 != losses1 and np.all(np.isfinite(losses0 + losses1))
    assert ex0['finish_calls'] == ex1['finish_calls'] == DITERS + DITERS // 2 and ex0['bytes_reduced'] == ex1['bytes_reduced']


# ------------------------------------------------------------------------------------------------ entry point
@pytest.mark.timeout(900)
def test_entry_point_trains_resumes_and_evaluates_with_the_shared_decoder(mrdis, tmp_path):
    """main_missing.py with shared_inp_dec: True on synthetic data: one epoch with its validation pass, a resumed second epoch, and the test
    phase from the saved checkpoint, each in a fresh process; then Run.evaluate with eval_info 'nearest_neighbour' in this process"""
    base = dict(contrast_list=['T1', 'T2'], input_height=64, input_width=64, batch_size=20, epochs=1, gpu='0', data_source='synthetic',
                ckpt_root=str(tmp_path / 'ckpt'), shared_inp_dec=True, lambda_adv_s=1.0)
    script = os.path.join(ROOT, 'main_missing.py')

    def run(name, cfg):
        (tmp_path / name).write_text(yaml.dump(cfg))
        r = subprocess.run([sys.executable, script, str(tmp_path / name)], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return r
    run('train.yaml', base)
    found = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path / 'ckpt')) for f in fs]
    assert any(f.endswith('model_best.pth.tar') for f in found), found
    sd = torch.load([f for f in found if f.endswith('model_best.pth.tar')][0], map_location='cpu', weights_only=False)['model']
    assert 'input_decoder_list.0.sp6.out.weight' in sd and not any(k.startswith('input_decoder_list.1.') for k in sd)
    stat = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path / 'ckpt')) for f in fs if f == 'stat.csv']
    label = os.path.basename(os.path.dirname(stat[0]))                  # the training run's directory (named by its start time)
    # resume from that checkpoint for a second epoch (load_yaml off: the saved config.yaml would put epochs back to 1)
    run('resume.yaml', dict(base, epochs=2, continue_train=True, ckpt_timelabel=label, load_yaml=False))
    rows = open(stat[0]).read().strip().split('\n')
    assert sum(r.split(',')[1] == 'val' for r in rows[1:]) == 2, rows
    r = run('test.yaml', dict(base, phase='test', ckpt_timelabel=label))
    assert 'psnr' in r.stdout, r.stdout[-2000:]

    store = mrdis.train.synthetic_store
    mrdis.train.synthetic_store = lambda config, device: store(config, device, n_subj=10)       # a test split of two subjects
    try:
        cfg = mrdis.train.setup_config(str(tmp_path / 'train.yaml'), device=DEV)
        cfg.update(batch_size=4, shuffle=False, ckpt_timelabel='t1')
        rn = mrdis.train.Run(cfg, log=lambda *a: None)
        assert rn.model.shared_inp_dec
        rn.train(max_iters_per_epoch=2)
        mrdis.hip.launch_counts(reset=True)
        stat = rn.evaluate(phase='test', set_='test', info='nearest_neighbour')
        assert mrdis.hip.launch_counts()['zsearch'] >= 2
        assert {'rmse', 'psnr', 'ssim', 'recon_x_mix', 'all'} <= set(stat) and np.isfinite(stat['all'])
    finally:
        mrdis.train.synthetic_store = store
