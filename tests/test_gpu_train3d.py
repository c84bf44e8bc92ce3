"""`Run3D` (train3d.py) on the GPU over a synthetic store: 32 x 32 x 123 volumes (Dz = 32 inside the reference's crop), four contrasts, NVNet3D with
init_channels 8, B = 2; the list files hold five / three / three subjects, of which the reference's reader serves four / two / two (it takes
the first line as a header, data3d.load_subj_list).

Fused against torch objective: the objective-parity margin, propagated through Adam.  tests/test_gpu_loss3d.py measures the fused gradients
within 2^-23 of their scale of the float64 values (so does the torch composition), and the fp32 backward pass keeps a perturbation at that
relative size.  An Adam step is lr m / (sqrt(v) + eps): it passes a RELATIVE change d of an element's gradient on as at most lr d, so n steps
from the same weights end about n lr 2^-23 apart on average (2.4e-11 for n = 2, lr 1e-4).  The perturbation is relative to the gradient's
scale, not to each element, so elements far below that scale see a larger relative change: CONDITIONING covers that factor, 100 with margin
(measured: 2.8).  The few elements whose gradient is itself at rounding level may flip sign and end up to 2 lr per step apart; they are bounded
by their share, not by a maximum distance: at most 1e-3 of the elements may be more than lr / 10 apart (a gradient wrong in sign or scale
would put most elements there).  The validation Dice of the two runs is a ratio of voxel counts over 2 x 3 x 32^3 voxels and must agree to 1e-4.
Measured on an MI355X (n = 2 steps, lr 1e-4; the test prints the line, profiles/loss3d_bench.txt records it): mean |dw| 6.7e-11 against the
asserted 2.4e-9, max |dw| 1.3e-06, no element beyond lr / 10, validation Dice equal to six digits; the weights themselves moved by 1.6e-04 on
average."""
import os

import numpy as np
import pytest
import torch

from fixtures_data3d import data3d_volumes, data3d_subjects

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
CONTRASTS = ['T1', 'T1c', 'T2', 'T2_FLAIR']
LR = 1e-4
CONDITIONING = 100                 # see the module docstring


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    """(store arrays, data_path with the three list files)"""
    data = data3d_volumes(n_subj=11, H=32, W=32, D=123, contrasts=CONTRASTS, seed=9)
    subj = data3d_subjects(data)
    root = tmp_path_factory.mktemp('data3d')
    for name, part in (('train', subj[:5]), ('val', subj[5:8]), ('test', subj[8:11])):
        (root / f'fold_BraTS_3d_0_{name}_noval.txt').write_text('\n'.join(part) + '\n')
    return data, str(root)


def _config(world, ckpt, **over):
    cfg = dict(dataset_name='BraTS', data_path=world[1], contrast_list=CONTRASTS, batch_size=2, model_name='NVNet3D', init_channels=8,
               epochs=2, lr=LR, lr_schedule='poly', ckpt_path=str(ckpt), device='cuda:0', seed=10)
    cfg.update(over)
    return cfg


def _run(mrdis, world, ckpt, **over):
    store = mrdis.VolumeStore3D.from_arrays(world[0], DEV)
    return mrdis.Run3D(_config(world, ckpt, **over), store=store, log=lambda *a: None)


def _weights(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def _flat(sd):
    return torch.cat([v.reshape(-1).double() for v in sd.values() if v.dtype.is_floating_point])


def test_fused_and_torch_objective_train_alike(mrdis, world, tmp_path):
    a = _run(mrdis, world, tmp_path / 'fused', epochs=1, fused_loss=True)
    c0 = mrdis.hip.launch_counts()['loss3d']
    w0 = _flat(_weights(a.model))
    a.train()
    n_steps = len(a.loaders['train'])
    assert n_steps == 2
    assert mrdis.hip.launch_counts()['loss3d'] == c0 + 2 * n_steps + len(a.loaders['val'])     # forward + backward per step, forward per validation batch
    b = _run(mrdis, world, tmp_path / 'torch', epochs=1, fused_loss=False)
    c1 = mrdis.hip.launch_counts()['loss3d']
    b.train()
    assert mrdis.hip.launch_counts()['loss3d'] == c1                                            # the torch composition launches none of them
    wa, wb = _flat(_weights(a.model)), _flat(_weights(b.model))
    d = (wa - wb).abs()
    moved = (wa - w0).abs()
    print(f'\n[run3d fused vs torch] {n_steps} steps, lr {LR:g}: max |dw| {float(d.max()):.3e}  mean |dw| {float(d.mean()):.3e}  '
          f'elements beyond lr/10: {float((d > LR / 10).double().mean()):.3e}  (weights moved: max {float(moved.max()):.3e} mean {float(moved.mean()):.3e})  '
          f'val dice fused {a.last_stat["dice"]:.6f} torch {b.last_stat["dice"]:.6f}')
    assert float(moved.mean()) > LR / 2                                                         # the epoch did train
    assert float(d.mean()) <= CONDITIONING * n_steps * LR * 2.0 ** -23
    assert float((d > LR / 10).double().mean()) <= 1e-3
    assert abs(a.last_stat['dice'] - b.last_stat['dice']) <= 1e-4 and abs(a.last_stat['iou'] - b.last_stat['iou']) <= 1e-4


def test_one_epoch_equals_the_readme_loop(mrdis, world, tmp_path):
    run = _run(mrdis, world, tmp_path / 'run', epochs=1, fused_loss=False, lr_schedule='none')
    run.train()
    # the README's hand-written loop, from the same seed
    torch.manual_seed(10); np.random.seed(10); torch.cuda.manual_seed(10)
    store = mrdis.VolumeStore3D.from_arrays(world[0], DEV)
    data = mrdis.VolumeData3D('BraTS', world[1], norm_type='z-score', batch_size=2, fold=0, shuffle=True, contrast_list=CONTRASTS, aug=True,
                              dropoff=True, store=store, device=DEV, region_channels=3)
    H, W, D = data.store.shape
    model = mrdis.NVNet3D((H, W, D - 91), 4, 3, 8, p=0.2).to(DEV).train()
    opt = mrdis.ArenaAdam(model.parameters(), lr=LR, weight_decay=1e-5)
    n = 0
    for batch in data.trainLoader:
        loss, parts = mrdis.nvnet_loss(*model(batch['inputs']), batch['inputs'], batch['targets'])
        loss.backward()
        opt.step(fused_clip=True)
        opt.zero_grad()
        n += 1
    assert n == 2
    got, want = run.model.state_dict(), model.state_dict()
    assert list(got) == list(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k


@pytest.fixture(scope='module')
def resumed(mrdis, world, tmp_path_factory):
    """two epochs straight, and one epoch + continue_train + one more, both with aug, drop-off and the fused objective"""
    d1, d2 = tmp_path_factory.mktemp('straight'), tmp_path_factory.mktemp('resumed')
    straight = _run(mrdis, world, d1).train()
    first = _run(mrdis, world, d2)
    first._train(1)                                  # an interrupted run: the schedule spans two epochs, one was trained
    assert sorted(f for f in os.listdir(d2) if f.startswith('epoch')) == ['epoch000.pth.tar']
    del first
    second = _run(mrdis, world, d2, continue_train=True)
    assert second.start_epoch == 0
    second.train()
    return straight, second, str(d1), str(d2)


def test_continue_train_is_bit_identical(mrdis, resumed):
    straight, second, d1, d2 = resumed
    a, b = straight.model.state_dict(), second.model.state_dict()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    oa, ob = straight.optimizer, second.optimizer
    for name in ('flat_p', 'm', 'v', 'vmax', 'step_state'):
        assert torch.equal(getattr(oa, name), getattr(ob, name)), name
    assert oa.lr == ob.lr and float(oa.step_state[0]) == 4
    assert straight.last_stat == second.last_stat
    ca = torch.load(os.path.join(d1, 'epoch001.pth.tar'), map_location='cpu', weights_only=False)
    cb = torch.load(os.path.join(d2, 'epoch001.pth.tar'), map_location='cpu', weights_only=False)
    assert ca['stat'] == cb['stat'] and ca['best_dice'] == cb['best_dice']
    assert torch.equal(ca['rng']['torch'], cb['rng']['torch']) and torch.equal(ca['rng']['device'], cb['rng']['device'])
    assert all(np.array_equal(p, q) for p, q in zip(ca['rng']['numpy'], cb['rng']['numpy']))
    for k in ('numpy', 'torch', 'device', 'loaders'):
        assert k in ca['rng']


def test_best_checkpoint_has_the_highest_dice_and_stat_csv(mrdis, resumed):
    _, _, d1, _ = resumed
    cks = [torch.load(os.path.join(d1, f'epoch{e:03d}.pth.tar'), map_location='cpu', weights_only=False) for e in range(2)]
    dices = [c['monitor_metric'] for c in cks]
    assert all(c['stat']['dice'] == c['monitor_metric'] and 0 < c['stat']['iou'] <= c['stat']['dice'] < 1 for c in cks)
    best = torch.load(os.path.join(d1, 'model_best.pth.tar'), map_location='cpu', weights_only=False)
    assert best['epoch'] == int(np.argmax(dices)) and best['monitor_metric'] == max(dices)
    for k in ('epoch', 'monitor_metric', 'stat', 'optimizer', 'scheduler', 'model', 'rng'):
        assert k in best
    rows = open(os.path.join(d1, 'stat.csv')).read().splitlines()
    assert sum('epoch[' in r for r in rows) == 2 and sum(',val,' in r for r in rows) == 2


def test_phase_test_runs_from_the_best_checkpoint(mrdis, world, resumed):
    _, _, d1, _ = resumed
    best = torch.load(os.path.join(d1, 'model_best.pth.tar'), map_location='cpu', weights_only=False)
    run = _run(mrdis, world, d1, phase='test')
    assert run.start_epoch == best['epoch']
    for k, v in best['model'].items():
        assert torch.equal(run.model.state_dict()[k].cpu(), v), k
    stat = run.evaluate('test')
    assert set(stat) == {'loss', 'loss_dice', 'loss_l2', 'loss_kl', 'dice', 'iou'} and all(np.isfinite(v) for v in stat.values())
    assert 0 < stat['iou'] <= stat['dice'] < 1


def test_validation_metrics_equal_seg_metrics_of_the_outputs(mrdis, world, tmp_path):
    run = _run(mrdis, world, tmp_path / 'val', epochs=1, dropoff=False)              # no drop-off: the validation batches draw nothing
    run.train()
    stat = run.last_stat
    before = mrdis.hip.launch_counts()['segcounts']
    run.model.eval()
    dice, iou = [], []
    with torch.no_grad():
        for batch in run.loaders['val']:
            m = mrdis.seg_metrics(run.model(batch['inputs'])[0], batch['targets'], logits=True)
            dice.append(m['dice']); iou.append(m['iou'])
    assert mrdis.hip.launch_counts()['segcounts'] == before + len(run.loaders['val'])
    dice, iou = torch.cat(dice), torch.cat(iou)
    assert dice.numel() == 2
    assert stat['dice'] == pytest.approx(float(dice.mean()), abs=1e-12) and stat['iou'] == pytest.approx(float(iou.mean()), abs=1e-12)
    # and against a plain torch count on the same outputs
    with torch.no_grad():
        for batch in run.loaders['val']:
            p = torch.sigmoid(run.model(batch['inputs'])[0]) > 0.5
            t = batch['targets'] == 1
            i_, p_, t_ = (p & t).sum((2, 3, 4)).double(), p.sum((2, 3, 4)).double(), t.sum((2, 3, 4)).double()
            want = ((2 * i_ + 1) / (t_ + p_ + 1)).mean(1).cpu()
    assert torch.allclose(want, dice, rtol=0, atol=1e-4)                         # (a logit within an ulp of 0 may count differently under torch's sigmoid)


def test_unet3d_dice_only_trains(mrdis, world, tmp_path):
    c0 = mrdis.hip.launch_counts()['loss3d']
    run = _run(mrdis, world, tmp_path / 'unet', epochs=1, model_name='UNet3D')
    run.train()
    assert mrdis.hip.launch_counts()['loss3d'] > c0
    assert run.last_stat['loss_l2'] == 0 and run.last_stat['loss_kl'] == 0 and 0 < run.last_stat['loss_dice'] < 1
    assert abs(run.last_stat['loss'] - run.last_stat['loss_dice']) < 1e-6
