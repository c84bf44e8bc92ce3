"""The fused objective of the 3-D nets and the segmentation counts (csrc/mrdis_loss3d.hip, model3d.nvnet_loss_hip / seg_metrics) on the GPU.

Objective parity has no tolerance fixed in advance: the yardstick is the existing fp32 `nvnet_loss` + autograd, measured against a float64
evaluation of the same formula in the same test.  The fused result's error against that float64 value (relative for the loss, max abs for the
gradients) may be at most 2 x the yardstick's -- the summation order differs -- with a floor of FLOOR_ULPS fp32 half-ulps of the value: the
fused value is one fp32 rounding of an fp64 evaluation on top of an fp32 sigmoid, so an error of a few half-ulps is what the number format
gives even where the yardstick happens to land closer.  Both errors are printed (tools/bench3d.py --loss-only prints them too, into
profiles/loss3d_bench.txt)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
FLOOR_ULPS = 4                     # floor of the margin: 4 * 2^-24 of the value's magnitude (see the module docstring)
EPS = 2.0 ** -24


def _cl3d(B, C, D, H, W, g, kind='randn'):
    """(B, C, D, H, W) fp32 on the device, channels-last-3d as the nets and the loader write it"""
    t = torch.randn(B, D, H, W, C, generator=g) if kind == 'randn' else (torch.rand(B, D, H, W, C, generator=g) > 0.7).float()
    return t.to(DEV).permute(0, 4, 1, 2, 3)


def _inputs(shape_u, shape_v, seed):
    g = torch.Generator().manual_seed(seed)
    uout, target = _cl3d(*shape_u, g), _cl3d(*shape_u, g, kind='mask')
    if shape_v is None:
        return uout, None, None, None, None, target
    vout, x = _cl3d(*shape_v, g), _cl3d(*shape_v, g)
    B = shape_u[0]
    mu, logvar = torch.randn(B, 16, generator=g).to(DEV), (0.1 * torch.randn(B, 16, generator=g)).to(DEV)
    return uout, vout, mu, logvar, x, target


def _dice_only(uout, target):
    p = torch.sigmoid(uout)
    return 1 - 2 * (p * target).sum() / ((p * p).sum() + (target * target).sum() + 1e-6)


def _evaluate(mrdis, fn, uout, vout, mu, logvar, x, target, dtype):
    """(loss, du, dv) of objective `fn` ('torch': nvnet_loss / the Dice term alone, 'fused': nvnet_loss_hip) with the inputs cast to dtype"""
    c = lambda t: None if t is None else t.detach().to(dtype)
    u = c(uout).requires_grad_(True)
    v = c(vout).requires_grad_(True) if vout is not None else None
    if fn == 'fused':
        loss, parts = mrdis.nvnet_loss_hip(u, v, c(mu), c(logvar), c(x), c(target))
        assert set(parts) == {'dice', 'l2', 'kl'}
    elif vout is None:
        loss = _dice_only(u, c(target))
    else:
        loss, parts = mrdis.nvnet_loss(u, v, c(mu), c(logvar), c(x), c(target))
    loss.backward()
    return loss.detach(), u.grad, (v.grad if v is not None else None)


def _errors(got, ref):
    l, du, dv = got
    l64, du64, dv64 = ref
    return (float(((l.double() - l64) / l64).abs()), float((du.double() - du64).abs().max()),
            float((dv.double() - dv64).abs().max()) if dv is not None else 0.0)


CASES = {
    'odd 2x3x24x40x56 + 2x4x24x40x56': ((2, 3, 24, 40, 56), (2, 4, 24, 40, 56)),
    'tails 1x3x5x7x9 + 1x5x5x7x9': ((1, 3, 5, 7, 9), (1, 5, 5, 7, 9)),                      # 945 and 1575 floats: n % 4 = 1 and 3
    'bench 4x3x128^3 + 4x4x128^3': ((4, 3, 128, 128, 128), (4, 4, 128, 128, 128)),
    'dice only 2x3x24x40x56': ((2, 3, 24, 40, 56), None),
    'dice only, tail 1x3x5x7x9': ((1, 3, 5, 7, 9), None),
}


@pytest.mark.parametrize('name', list(CASES))
def test_objective_matches_float64_within_twice_the_torch_error(mrdis, name):
    shape_u, shape_v = CASES[name]
    args = _inputs(shape_u, shape_v, seed=4)
    ref = _evaluate(mrdis, 'torch', *args, dtype=torch.float64)
    e_torch = _errors(_evaluate(mrdis, 'torch', *args, dtype=torch.float32), ref)
    before = mrdis.hip.launch_counts()['loss3d']
    fused = _evaluate(mrdis, 'fused', *args, dtype=torch.float32)
    assert mrdis.hip.launch_counts()['loss3d'] == before + 2                    # the HIP kernels ran: one forward, one backward
    e_fused = _errors(fused, ref)
    assert fused[1].stride() == args[0].stride() and (fused[2] is None or fused[2].stride() == args[1].stride())
    scale = (1.0, float(ref[1].abs().max()), float(ref[2].abs().max()) if ref[2] is not None else 0.0)
    print(f'\n[loss3d parity] {name}: loss {float(ref[0]):.9f}  |du|max {scale[1]:.3e}  |dv|max {scale[2]:.3e}')
    for what, et, ef, s in zip(('loss rel', 'du max abs', 'dv max abs'), e_torch, e_fused, scale):
        bound = max(2 * et, FLOOR_ULPS * EPS * s)
        print(f'[loss3d parity]   {what}: torch fp32 {et:.3e}  fused {ef:.3e}  bound {bound:.3e}')
    for what, et, ef, s in zip(('loss rel', 'du max abs', 'dv max abs'), e_torch, e_fused, scale):
        assert ef <= max(2 * et, FLOOR_ULPS * EPS * s), (name, what, ef, et)


def test_parts_match_nvnet_loss(mrdis):
    args = _inputs((2, 3, 8, 16, 24), (2, 4, 8, 16, 24), seed=5)
    loss, parts = mrdis.nvnet_loss(*args)
    loss_h, parts_h = mrdis.nvnet_loss_hip(*args)
    assert list(parts_h) == list(parts)
    for k in parts:
        assert parts_h[k].shape == parts[k].shape == () and parts_h[k].dtype == torch.float32
        assert float(parts_h[k]) == pytest.approx(float(parts[k]), rel=1e-5), k
    assert float(loss_h) == pytest.approx(float(loss), rel=1e-5)


def test_two_calls_are_bit_identical_and_counted(mrdis):
    args = _inputs((2, 3, 24, 40, 56), (2, 4, 24, 40, 56), seed=6)
    uout, vout, mu, logvar, x, target = args
    hip = mrdis.hip
    c0 = hip.launch_counts()['loss3d']
    u = uout.detach().requires_grad_(True); v = vout.detach().requires_grad_(True)
    loss, _ = mrdis.nvnet_loss_hip(u, v, mu, logvar, x, target)
    assert hip.launch_counts()['loss3d'] == c0 + 1                              # forward: + 1
    loss.backward()
    assert hip.launch_counts()['loss3d'] == c0 + 2                              # backward: + 1
    a = _evaluate(mrdis, 'fused', *args, dtype=torch.float32)
    b = _evaluate(mrdis, 'fused', *args, dtype=torch.float32)
    for p, q in zip(a, b):
        assert torch.equal(p, q)
    assert torch.equal(a[0], loss.detach()) and torch.equal(a[1], u.grad) and torch.equal(a[2], v.grad)
    s1, t1 = hip.nvnet_loss_fwd(uout, target, vout, x)
    s2, t2 = hip.nvnet_loss_fwd(uout, target, vout, x)
    assert s1.dtype == torch.float64 and torch.equal(s1, s2) and torch.equal(t1, t2)
    p = torch.sigmoid(uout.double())
    want = torch.stack([(p * target).sum(), (p * p).sum(), (target.double() ** 2).sum(), ((vout.double() - x.double()) ** 2).sum()])
    assert float(((s1 - want) / want).abs().max()) <= 1e-6


def test_layout_mismatch_and_holes_raise(mrdis):
    uout, vout, mu, logvar, x, target = _inputs((2, 3, 8, 16, 24), (2, 4, 8, 16, 24), seed=7)
    with pytest.raises(mrdis.MrdisError):                                       # target NCDHW-contiguous, uout channels-last-3d: no silent copy
        mrdis.nvnet_loss_hip(uout, vout, mu, logvar, x, target.contiguous())
    with pytest.raises(mrdis.MrdisError):
        mrdis.nvnet_loss_hip(uout, vout.contiguous(), mu, logvar, x, target)
    with pytest.raises(mrdis.MrdisError):                                       # same strides on both sides, but not dense
        mrdis.nvnet_loss_hip(uout[:, :, ::2], vout, mu, logvar, x, target[:, :, ::2])
    with pytest.raises(mrdis.MrdisError):
        mrdis.nvnet_loss_hip(uout[:, :2], vout, mu, logvar, x, target[:, :2])
    with pytest.raises(mrdis.MrdisError):
        mrdis.nvnet_loss_hip(uout, vout, mu, logvar, x, target[:1])
    with pytest.raises(mrdis.MrdisError):
        mrdis.nvnet_loss_hip(uout.double(), vout, mu, logvar, x, target.double())
    # any dense layout shared by a pair is taken as it is
    a = mrdis.nvnet_loss_hip(uout, vout, mu, logvar, x, target)[0]
    b = mrdis.nvnet_loss_hip(uout.contiguous(), vout.contiguous(), mu, logvar, x.contiguous(), target.contiguous())[0]
    assert float(a) == pytest.approx(float(b), rel=1e-6)


def _region_channels(labels):
    t = torch.stack([(labels == c + 1).float() for c in range(3)], 1)
    return t.to(DEV).contiguous(memory_format=torch.channels_last_3d)


def test_seg_metrics_equal_the_reference(mrdis, golden_dir):
    g = np.load(os.path.join(golden_dir, 'segmetrics3d.npz'))
    pred = torch.from_numpy(g['pred']).to(DEV).contiguous(memory_format=torch.channels_last_3d)
    target = _region_channels(torch.from_numpy(g['labels']))
    before = mrdis.hip.launch_counts()['segcounts']
    m = mrdis.seg_metrics(pred, target, logits=False)
    assert mrdis.hip.launch_counts()['segcounts'] == before + 1
    assert m['dice'].dtype == torch.float64 and tuple(m['dice'].shape) == (3,)
    assert np.abs(m['dice'].numpy() - g['dice']).max() <= 1e-12 and np.abs(m['iou'].numpy() - g['iou']).max() <= 1e-12
    # NCDHW-contiguous inputs give the same counts
    m2 = mrdis.seg_metrics(pred.contiguous(), target.contiguous(), logits=False)
    assert torch.equal(m2['dice'], m['dice']) and torch.equal(m2['iou'], m['iou'])
    # logits: agree wherever no prediction sits at the threshold (those within 1e-3 of it are moved away first)
    p = torch.from_numpy(g['pred']).double()
    p = torch.where((p - 0.5).abs() < 1e-3, torch.full_like(p, 0.4), p).clamp(1e-6, 1 - 1e-6)
    pf = p.float().to(DEV).contiguous(memory_format=torch.channels_last_3d)
    lg = torch.logit(p).float().to(DEV).contiguous(memory_format=torch.channels_last_3d)
    ma, mb = mrdis.seg_metrics(pf, target, logits=False), mrdis.seg_metrics(lg, target, logits=True)
    assert torch.equal(ma['dice'], mb['dice']) and torch.equal(ma['iou'], mb['iou'])


@pytest.mark.parametrize('shape', [(2, 3, 5, 7, 9), (2, 3, 8, 8, 8), (3, 2, 1, 2, 3), (1, 4, 6, 10, 7), (2, 1, 3, 5, 7), (1, 3, 32, 48, 64)])
def test_seg_counts_are_exact(mrdis, shape):
    """every channel count and both load forms (16-byte and 4-byte; a last group of fewer than four positions) against torch's own counting"""
    g = torch.Generator().manual_seed(8)
    B, C, D, H, W = shape
    logits = torch.randn(B, D, H, W, C, generator=g).to(DEV).permute(0, 4, 1, 2, 3)
    target = (torch.rand(B, D, H, W, C, generator=g) > 0.6).float().to(DEV).permute(0, 4, 1, 2, 3)
    for lg in (True, False):
        pred = logits if lg else torch.sigmoid(logits)
        got = mrdis.hip.seg_counts(pred, target, logits=lg)
        pp, tt = torch.sigmoid(logits) > 0.5, target == 1
        want = torch.stack([(pp & tt).sum((2, 3, 4)), pp.sum((2, 3, 4)), tt.sum((2, 3, 4))], -1).to(torch.int32)
        assert got.dtype == torch.int32 and tuple(got.shape) == (B, C, 3)
        assert torch.equal(got, want), (shape, lg)
