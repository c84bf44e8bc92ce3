"""CPU-side checks of the 3-D training entry (train3d.py, main_3d.py) and of what the segmentation metrics are made of: the reference's
formulas against its recorded results (tests/golden/segmetrics3d.npz, tools/gen_golden_seg3d.py), config parsing, the poly schedule, the ABI
declarations and the refusal under a process group.  Nothing here touches a GPU."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'segmetrics3d.npz')


def golden_counts(labels, pred):
    """(B, 3, 3) integer counts [I, P, T] taken from the golden's inputs: channel c against label c + 1, prediction strictly above 0.5"""
    B = labels.shape[0]
    out = np.zeros((B, 3, 3), dtype=np.int64)
    for b in range(B):
        for c in range(3):
            t, p = labels[b] == c + 1, pred[b, c] > 0.5
            out[b, c] = [(t & p).sum(), p.sum(), t.sum()]
    return out


def test_golden_case_has_the_edge_cases():
    g = np.load(GOLDEN)
    labels, pred = g['labels'], g['pred']
    assert labels.shape == (3, 8, 8, 8) and pred.shape == (3, 3, 8, 8, 8) and pred.dtype == np.float32
    assert any((labels[b] == c + 1).sum() == 0 for b in range(3) for c in range(3))         # a class absent from one sample
    assert (pred == 0.5).sum() > 0                                                            # predictions exactly at the threshold
    assert any((pred[b] > 0.5).sum() == 0 for b in range(3))                                  # one empty prediction
    assert os.path.getsize(GOLDEN) < 64 * 1024


def test_metric_formulas_reproduce_the_reference():
    """numpy restatement of dice_c = (2 I + 1) / (T + P + 1), iou_c = (I + 1) / (T + P - I + 1), mean over the three channels"""
    g = np.load(GOLDEN)
    c = golden_counts(g['labels'], g['pred']).astype(np.float64)
    i, p, t = c[..., 0], c[..., 1], c[..., 2]
    dice = ((2 * i + 1) / (t + p + 1)).mean(1)
    iou = ((i + 1) / (t + p - i + 1)).mean(1)
    assert np.abs(dice - g['dice']).max() <= 1e-12 and np.abs(iou - g['iou']).max() <= 1e-12


def test_seg_metrics_from_counts_reproduces_the_reference():
    import mrdis
    g = np.load(GOLDEN)
    m = mrdis.model3d.seg_metrics_from_counts(golden_counts(g['labels'], g['pred']))
    assert m['dice'].dtype == torch.float64 and tuple(m['dice'].shape) == (3,) and tuple(m['iou'].shape) == (3,)
    assert np.abs(m['dice'].numpy() - g['dice']).max() <= 1e-12 and np.abs(m['iou'].numpy() - g['iou']).max() <= 1e-12


def test_config_defaults_and_example_file():
    import mrdis
    t3 = mrdis.train3d
    cfg = t3.load_config3d()
    assert cfg == t3.DEFAULT_CONFIG_3D and cfg is not t3.DEFAULT_CONFIG_3D
    for k in ('dataset_name', 'data_path', 'norm_type', 'fold', 'contrast_list', 'batch_size', 'model_name', 'init_channels', 'p', 'aug', 'dropoff',
              'epochs', 'lr', 'weight_decay', 'lr_schedule', 'fused_loss', 'ckpt_path', 'continue_train', 'phase', 'seed', 'device', 'max_batches'):
        assert k in cfg, k
    assert cfg['fused_loss'] is True and cfg['model_name'] == 'NVNet3D' and cfg['phase'] == 'train' and cfg['lr_schedule'] == 'poly'
    assert t3.load_config3d(os.path.join(ROOT, 'config3d.yaml')) == t3.DEFAULT_CONFIG_3D        # the commented example states the defaults


def test_command_line_overrides(tmp_path):
    import mrdis
    t3 = mrdis.train3d
    f = tmp_path / 'c.yaml'
    f.write_text('epochs: 7\nmodel_name: UNet3D\n')
    path, ov = t3.parse_argv([str(f), 'epochs=2', 'lr=1e-3', 'contrast_list=[T1,T2]', 'fused_loss=false', 'lr_schedule=none', 'max_batches=3'])
    assert path == str(f)
    cfg = t3.load_config3d(path, ov)
    assert cfg['epochs'] == 2 and cfg['model_name'] == 'UNet3D' and cfg['lr'] == 1e-3 and isinstance(cfg['lr'], float)
    assert cfg['contrast_list'] == ['T1', 'T2'] and cfg['fused_loss'] is False and cfg['lr_schedule'] == 'none' and cfg['max_batches'] == 3
    assert t3.parse_argv(['phase=test']) == (None, {'phase': 'test'})
    with pytest.raises(KeyError):
        t3.load_config3d(None, {'no_such_key': 1})
    for bad in ({'model_name': 'VGG'}, {'lr_schedule': 'cosine'}, {'phase': 'val'}):
        with pytest.raises(ValueError):
            t3.load_config3d(None, bad)
    src = open(os.path.join(ROOT, 'main_3d.py')).read()
    assert 'mrdis.train3d.main()' in src


def test_poly_schedule():
    import mrdis
    t3 = mrdis.train3d
    assert t3.poly_lr(1e-4, 0, 10) == 1e-4
    for e, E in ((1, 10), (5, 10), (9, 10), (150, 300)):
        assert t3.poly_lr(2e-4, e, E) == pytest.approx(2e-4 * (1 - e / E) ** 0.9, rel=1e-15)
    lrs = [t3.epoch_lr({'lr': 1e-4, 'epochs': 4, 'lr_schedule': 'poly'}, e) for e in range(4)]
    assert lrs == sorted(lrs, reverse=True) and lrs[-1] > 0
    assert [t3.epoch_lr({'lr': 1e-4, 'epochs': 4, 'lr_schedule': 'none'}, e) for e in range(4)] == [1e-4] * 4


def test_resume_picks_the_highest_epoch_by_number(tmp_path):
    import mrdis
    t3 = mrdis.train3d
    with pytest.raises(ValueError):
        t3.last_epoch_checkpoint(str(tmp_path))
    for name in ('epoch000.pth.tar', 'epoch999.pth.tar', 'model_best.pth.tar', 'epochs.txt'):
        (tmp_path / name).write_text('')
    assert t3.last_epoch_checkpoint(str(tmp_path)) == 'epoch999.pth.tar'
    (tmp_path / 'epoch1000.pth.tar').write_text('')                          # sorts before 'epoch999' as a string
    assert t3.last_epoch_checkpoint(str(tmp_path)) == 'epoch1000.pth.tar'


def test_new_abi_symbols_are_declared_bound_and_exported():
    import mrdis
    txt = open(os.path.join(ROOT, 'include', 'mrdis.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    declared = set(re.findall(r'\b(mrdis_[a-z0-9_]+)\s*\(', txt))
    lib = mrdis.hip.load()
    for name in ('mrdis_nvnet_loss_workspace', 'mrdis_nvnet_loss_fwd', 'mrdis_nvnet_loss_bwd', 'mrdis_seg_counts'):
        assert name in declared, f'{name} not declared in include/mrdis.h'
        assert name in mrdis.hip.EXPORTED_SYMBOLS and hasattr(lib, name), name
    # host-only calls: the workspace is a pure function of the element counts, the new counters are names the library knows
    assert lib.mrdis_nvnet_loss_workspace(4 * 3 * 128 ** 3, 4 * 4 * 128 ** 3) >= 32
    assert lib.mrdis_nvnet_loss_workspace(0, 0) == 0
    for fam in mrdis.hip.LOSS3D_FAMILIES:
        assert lib.mrdis_launch_count(fam.encode()) >= 0, fam
    assert set(mrdis.hip.LOSS3D_FAMILIES) == {'loss3d', 'segcounts'} <= set(mrdis.hip.launch_counts())
    assert mrdis.Run3D is mrdis.train3d.Run3D and callable(mrdis.nvnet_loss_hip) and callable(mrdis.seg_metrics)


def test_run3d_refuses_a_process_group(tmp_path):
    import torch.distributed as dist
    import mrdis
    assert not dist.is_initialized()
    dist.init_process_group('gloo', init_method=f'file://{tmp_path}/pg', rank=0, world_size=1)
    try:
        with pytest.raises(NotImplementedError, match='world size 1'):
            mrdis.Run3D({'ckpt_path': str(tmp_path / 'ck'), 'device': 'cpu'})
    finally:
        dist.destroy_process_group()
    assert not os.path.exists(tmp_path / 'ck')
