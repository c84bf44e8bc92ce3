"""The output decoders 'U', 'U+SA+CA' and 'U+SSA+CA' on the MI355X: the new kernels of csrc/mrdis_outdec.hip (channel attention with the skip
sum, symmetric difference, residual gate) against float64, forward and backward, and one training step of each decoder against the real
reference (tools/gen_golden_outdec.py): loss, gradient norms, weights after Adam, and the launch counters of the kernels that ran."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fixtures import make_inputs, make_seg_targets
from fixtures_outdec import make_float_targets

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def cl(x):
    return x.to(DEV).contiguous(memory_format=torch.channels_last)


def _slice(B, C, H, W, pad, seed):
    """a (B, C, H, W) channel slice [pad, pad + C) of a channels_last buffer with C + 2 pad channels, filled with N(0, 1)"""
    g = torch.Generator().manual_seed(seed)
    buf = cl(torch.randn(B, C + 2 * pad, H, W, generator=g))
    return buf[:, pad:pad + C]


def _err(got, want):
    want = want.double().cpu()
    return float((got.double().cpu() - want).abs().max()) / (float(want.abs().max()) + 1e-30)


# ------------------------------------------------------------------------------------------- kernels against float64
@pytest.mark.parametrize('C', [64, 128, 256, 512])
@pytest.mark.parametrize('HW', [(10, 12), (8, 8), (64, 64)], ids=str)
def test_channel_attention_kernel_vs_float64(mrdis, C, HW):
    H, W = HW
    B, Hd = 3, 64
    hip = mrdis.hip
    x, s, dy = _slice(B, C, H, W, 4, 1), _slice(B, C, H, W, 0, 2), _slice(B, C, H, W, 8, 3)
    g = torch.Generator().manual_seed(4)
    wd, bd = (torch.randn(Hd, C, generator=g) / C ** 0.5).to(DEV), (0.1 * torch.randn(Hd, generator=g)).to(DEV)
    wu, bu = (torch.randn(C, Hd, generator=g) / Hd ** 0.5).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)
    out_buf = cl(torch.full((B, 2 * C, H, W), 7.0))
    hip.launch_counts(reset=True)
    y1, pool, hid, a = hip.chatt_fwd(x, s, wd, bd, wu, bu, out=out_buf[:, :C])
    y1c = out_buf[:, :C].clone()
    assert torch.equal(out_buf[:, C:], torch.full_like(out_buf[:, C:], 7.0))        # nothing outside the slice
    y2, *_ = hip.chatt_fwd(x, s, wd, bd, wu, bu)
    assert torch.equal(y1c, y2)                                                      # bit-identical, slice or not
    grads = hip.chatt_bwd(dy, x, a, hid, pool, wd, wu)
    grads2 = hip.chatt_bwd(dy, x, a, hid, pool, wd, wu)
    assert all(torch.equal(u, v) for u, v in zip(grads, grads2))
    assert hip.launch_counts()['chatt'] == 4

    X = x.detach().double().cpu().requires_grad_()
    Wd, Bd, Wu, Bu = (t.double().cpu().requires_grad_() for t in (wd, bd, wu, bu))
    S = s.double().cpu()
    A = torch.sigmoid(F.relu(X.mean((2, 3)) @ Wd.T + Bd) @ Wu.T + Bu)
    Y = (1 + A[:, :, None, None]) * X + S
    Y.backward(dy.double().cpu())
    assert _err(y1c, Y.detach()) <= 2e-6
    assert _err(a, A.detach()) <= 2e-6
    for got, want, tol in zip(grads, (X.grad, Wd.grad, Bd.grad, Wu.grad, Bu.grad), (2e-6, 5e-5, 5e-5, 5e-5, 5e-5)):
        assert _err(got, want) <= tol, (got.shape, _err(got, want))


def test_channel_attention_scalar_form(mrdis):
    """C not a multiple of 4 and an odd channel offset: the scalar forms"""
    hip = mrdis.hip
    B, C, H, W, Hd = 2, 6, 5, 6, 3
    x, s, dy = _slice(B, C, H, W, 1, 5), _slice(B, C, H, W, 1, 6), _slice(B, C, H, W, 1, 7)
    g = torch.Generator().manual_seed(8)
    wd, bd, wu, bu = (torch.randn(*sh, generator=g).to(DEV) for sh in ((Hd, C), (Hd,), (C, Hd), (C,)))
    y, pool, hid, a = hip.chatt_fwd(x, s, wd, bd, wu, bu)
    dx, dwd, dbd, dwu, dbu = hip.chatt_bwd(dy, x, a, hid, pool, wd, wu)
    X = x.detach().double().cpu().requires_grad_()
    Wd, Bd, Wu, Bu = (t.double().cpu().requires_grad_() for t in (wd, bd, wu, bu))
    Y = (1 + torch.sigmoid(F.relu(X.mean((2, 3)) @ Wd.T + Bd) @ Wu.T + Bu)[:, :, None, None]) * X + s.double().cpu()
    Y.backward(dy.double().cpu())
    assert _err(y, Y.detach()) <= 2e-6
    for got, want in zip((dx, dwd, dbd, dwu, dbu), (X.grad, Wd.grad, Bd.grad, Wu.grad, Bu.grad)):
        assert _err(got, want) <= 5e-5


@pytest.mark.parametrize('C', [64, 128, 256, 512, 6])
@pytest.mark.parametrize('HW', [(5, 6), (8, 8), (64, 64)], ids=str)
def test_symmetric_difference_kernel_vs_float64(mrdis, C, HW):
    H, W = HW
    B = 2
    hip = mrdis.hip
    gt, dgd = _slice(B, C, H, W, 4 if C % 4 == 0 else 1, 11), _slice(B, C, H, W, 0, 12)
    hip.launch_counts(reset=True)
    out = cl(torch.zeros(B, C + 8, H, W))[:, 8:]
    gd = hip.symdiff_fwd(gt, out=out)
    G = gt.detach().double().cpu().requires_grad_()
    GD = (G - torch.flip(G, dims=[2])).abs()
    GD.backward(dgd.double().cpu())
    assert torch.equal(gd.cpu().double(), GD.detach().float().double())               # exact: one subtraction, one abs
    dg = hip.symdiff_bwd(dgd, gt)
    assert torch.equal(dg, hip.symdiff_bwd(dgd, gt))
    assert _err(dg, G.grad) <= 1e-6
    if H % 2:
        assert float(dg[:, :, H // 2].abs().max()) == 0.0                            # sgn(0) = 0 on the middle row
    assert hip.launch_counts()['symdiff'] == 3


@pytest.mark.parametrize('C', [64, 128, 256, 512, 6])
@pytest.mark.parametrize('HW', [(5, 6), (8, 8), (64, 64)], ids=str)
def test_residual_gate_kernel_vs_float64(mrdis, C, HW):
    """HW: the gate's (alpha's) resolution; x is twice that"""
    h, w = HW
    B, H, W = 2, 2 * h, 2 * w
    hip = mrdis.hip
    x, dy = _slice(B, C, H, W, 4 if C % 4 == 0 else 1, 21), _slice(B, C, H, W, 0, 22)
    alpha = torch.sigmoid(torch.randn(B, 1, h, w, generator=torch.Generator().manual_seed(23))).to(DEV)
    hip.launch_counts(reset=True)
    y = hip.rgate_fwd(x, alpha)
    dx, dal = hip.rgate_bwd(dy, x, alpha)
    dx2, dal2 = hip.rgate_bwd(dy, x, alpha)
    assert torch.equal(dx, dx2) and torch.equal(dal, dal2) and torch.equal(y, hip.rgate_fwd(x, alpha))
    assert hip.launch_counts()['rgate'] == 4
    X = x.detach().double().cpu().requires_grad_()
    A = alpha.double().cpu().requires_grad_()
    Y = (1 + F.interpolate(A, size=(H, W), mode='bilinear', align_corners=False)) * X
    Y.backward(dy.double().cpu())
    assert _err(y, Y.detach()) <= 2e-6
    assert _err(dx, X.grad) <= 2e-6
    assert _err(dal, A.grad) <= 2e-5


# ------------------------------------------------------------------------------------------- one training step against the reference
STEP_TAGS = ['b2m2_u', 'b2m2_uca', 'b2m2_ussaca', 'b2m2_ussaca_sp']


def _cfg(mrdis, meta, **kw):
    cfg = dict(mrdis.DEFAULT_CONFIG)
    cfg.update(contrast_list=[f'm{i}' for i in range(meta['M'])], input_height=meta['H'], input_width=meta['W'], batch_size=16,
               lambda_recon_y=meta['lambdas']['recon_y'], out_num_ch=meta['out_num_ch'], target_model_name=meta['target_model_name'],
               fuse_method=meta['fuse_method'], dataset_name=meta['dataset_name'], norm_type=meta['norm_type'])
    cfg.update(kw)
    return mrdis.derive_config(cfg, DEV)


def _targets(meta):
    B, H, W = meta['B'], meta['H'], meta['W']
    if meta['dataset_name'] == 'BraTS':
        return make_seg_targets(B, H, W, seed=meta['target_seed'])
    return make_float_targets(B, H, W, seed=meta['target_seed'])


@pytest.mark.parametrize('tag', STEP_TAGS)
def test_train_step_golden_output_decoders(mrdis, golden_dir, tag):
    meta = json.load(open(os.path.join(golden_dir, f'step_{tag}.json')))
    arrs = np.load(os.path.join(golden_dir, f'step_{tag}.npz'))
    grad_norms = dict(zip(arrs['grad_names'].tolist(), arrs['grad_norms'].tolist()))
    wsum_before = dict(zip(arrs['wsum_names'].tolist(), arrs['wsum_before'].tolist()))
    wsum_after = dict(zip(arrs['wsum_names'].tolist(), arrs['wsum_after'].tolist()))
    B, M, H, W = meta['B'], meta['M'], meta['H'], meta['W']
    cfg = _cfg(mrdis, meta)
    torch.manual_seed(10); np.random.seed(10)
    model = mrdis.build_model(cfg).train()
    for k, v in wsum_before.items():
        got = float(model.state_dict()[k].double().sum())
        assert abs(got - v) <= 1e-6 * max(1.0, abs(v)), ('init', k)
    inputs, mask, mask_img = make_inputs(B, M, H, W, seed=10, drop=False)
    targets = _targets(meta)
    step = mrdis.TrainStep(model, cfg)
    torch.manual_seed(11); np.random.seed(11)
    names = {id(p): n for n, p in model.named_parameters()}
    mrdis.hip.launch_counts(reset=True)
    with mrdis.ops.mix_cache():
        loss, parts, aux = mrdis.forward_losses(model, cfg, cl(inputs), mask.to(DEV), mask_img.to(DEV), mask, targets=targets.to(DEV))
        loss.backward()
    counts = mrdis.hip.launch_counts()
    name = meta['target_model_name']
    assert (counts['chatt'] > 0) == ('CA' in name), counts
    assert (counts['symdiff'] > 0) == (counts['rgate'] > 0) == ('SSA' in name), counts
    assert abs(float(loss) - meta['loss']) <= 1e-3 * abs(meta['loss'])
    for k, v in meta['parts'].items():
        assert abs(float(parts[k]) - v) <= 1e-3 * abs(v) + 1e-6, (k, float(parts[k]), v)
    for i in range(M):
        want = arrs[f'y{i}_pool8']
        got = F.avg_pool2d(aux['y_list'][i], 8).detach().float().cpu()
        assert float((got - torch.as_tensor(want)).abs().max()) <= 2e-3 * float(np.abs(want).max()) + 1e-7, f'y{i}'
    gn = {names[id(p)]: float(p.grad.double().norm()) for p in model.parameters() if p.grad is not None}
    assert set(grad_norms) == set(gn) and len(gn) == meta['n_params_with_grad']
    total = float(np.sqrt(sum(v * v for v in gn.values())))
    assert abs(total - meta['grad_norm']) <= 1e-3 * meta['grad_norm'], (total, meta['grad_norm'])
    for k, v in grad_norms.items():
        assert abs(gn[k] - v) <= 5e-3 * v + 2e-5 * meta['grad_norm'], (k, gn[k], v)
    step.optimizer.step(fused_clip=True)
    for k, v in wsum_after.items():
        if grad_norms.get(k, 1.0) < 1e-5 * meta['grad_norm']:
            continue
        t = model.state_dict()[k]
        got = float(t.double().sum())
        flips = 2 * cfg['lr'] * np.ceil(1e-3 * t.numel())
        assert abs(got - v) <= 2e-4 * max(1.0, abs(v)) + flips, ('after step', k, got, v)


def test_graph_replay_ussaca_non_brats_is_bit_identical(mrdis, golden_dir):
    """'U+SSA+CA' with the softplus activations and the p = 1 recon-y loss: the graph-replayed step equals the eager step bit for bit"""
    meta = json.load(open(os.path.join(golden_dir, 'step_b2m2_ussaca_sp.json')))
    B, M, H, W = 2, 2, 64, 96
    res = {}
    for graph in (False, True):
        cfg = _cfg(mrdis, dict(meta, M=M, H=H, W=W))
        torch.manual_seed(10); np.random.seed(10)
        model = mrdis.build_model(cfg).train()
        step = mrdis.TrainStep(model, cfg)
        if graph:
            step = mrdis.GraphedTrainStep(step)
        torch.manual_seed(100); np.random.seed(100)
        losses = []
        for it in range(5):
            x, mask, mask_img = mrdis.synthetic_batch(B, M, H, W, seed=40 + it)
            tg = make_float_targets(B, H, W, seed=60 + it).to(DEV)
            loss, _, _ = step(cl(x), mask.to(DEV), mask_img.to(DEV), mask, targets=tg)
            losses.append(float(loss))
        torch.cuda.synchronize()
        if graph:
            assert step.stats['replays'] > 0, step.stats
        res[graph] = (losses, torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu())
    assert res[True][0] == res[False][0]
    assert torch.equal(res[True][1], res[False][1])


@pytest.mark.parametrize('name', ['U+SA+CA', 'U+SSA+CA'])
def test_bf16m_runs_the_attention_decoders(mrdis, golden_dir, name):
    meta = json.load(open(os.path.join(golden_dir, 'step_b2m2_uca.json')))
    B, M, H, W = 2, 2, 64, 96
    cfg = _cfg(mrdis, dict(meta, M=M, H=H, W=W, target_model_name=name), compute_dtype='bf16m')
    try:
        torch.manual_seed(10); np.random.seed(10)
        model = mrdis.build_model(cfg).train()
        step = mrdis.TrainStep(model, cfg)
        x, mask, mask_img = mrdis.synthetic_batch(B, M, H, W, seed=3)
        before = {n: p.detach().clone() for n, p in model.named_parameters() if n.startswith('output_decoder.att_')}
        mrdis.hip.launch_counts(reset=True)
        loss, _, _ = step(cl(x), mask.to(DEV), mask_img.to(DEV), mask, targets=make_seg_targets(B, H, W, seed=13).to(DEV))
        assert np.isfinite(float(loss))
        assert mrdis.hip.launch_counts()['chatt'] > 0
        moved = [n for n, p in model.named_parameters() if n in before and not torch.equal(before[n], p.detach())]
        assert any('_c.W_down' in n for n in moved) and any('_s.W_out' in n for n in moved), moved
    finally:
        mrdis.ops.set_compute_dtype('f32')
