"""Host side of the whole-volume sliding-window prediction (model3d.window_offsets, the `phase: predict` configuration): no GPU."""
import os

import pytest
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def mrdis():
    import mrdis as m
    return m


def test_window_offsets(mrdis):
    wo = mrdis.window_offsets
    assert wo(155, 64, 32) == [0, 32, 64, 91]                     # BraTS: the last window ends at the last slice, odd offset
    assert wo(123, 32, 16) == [0, 16, 32, 48, 64, 80, 91]
    assert wo(123, 32, 16)[-1] == 91
    assert wo(64, 64, 32) == [0] and wo(64, 64, 1) == [0]         # D == Dz: one window
    assert wo(96, 32, 32) == [0, 32, 64]                          # the last regular offset IS D - Dz: no duplicate
    assert wo(97, 32, 32) == [0, 32, 64, 65]
    assert wo(37, 16, 8) == [0, 8, 16, 21]
    for D, Dz, s in ((155, 64, 32), (123, 32, 16), (37, 16, 8), (50, 7, 3)):
        off = wo(D, Dz, s)
        assert off == sorted(set(off)) and off[0] == 0 and off[-1] == D - Dz
        assert all(b - a <= s for a, b in zip(off, off[1:]))


def test_window_offsets_stride_above_the_window_leaves_gaps(mrdis):
    off = mrdis.window_offsets(100, 10, 40)
    assert off == [0, 40, 80, 90]
    cover = mrdis.model3d.window_cover(100, 10, off, flips=2)
    assert cover.dtype.name == 'int32' and cover.shape == (100,)
    assert cover[:10].tolist() == [2] * 10 and cover[10:40].tolist() == [0] * 30                 # uncovered depths
    assert cover[80:90].tolist() == [2] * 10 and cover[90:].tolist() == [2] * 10
    assert mrdis.model3d.window_cover(37, 16, [0, 8, 16, 21]).tolist() == [1] * 8 + [2] * 13 + [3] * 3 + [2] * 8 + [1] * 5


def test_window_offsets_errors(mrdis):
    with pytest.raises(ValueError):
        mrdis.window_offsets(63, 64, 32)                          # D < Dz
    with pytest.raises(ValueError):
        mrdis.window_offsets(155, 64, 0)
    with pytest.raises(ValueError):
        mrdis.window_offsets(155, 64, -3)


def test_config_accepts_phase_predict_and_its_keys(mrdis):
    t3 = mrdis.train3d
    cfg = t3.load_config3d(None, {})
    assert cfg['predict_set'] == 'test' and cfg['predict_stride'] is None and cfg['predict_flip'] is False
    cfg = t3.load_config3d(None, {'phase': 'predict', 'predict_set': 'val', 'predict_stride': 16, 'predict_flip': True})
    assert cfg['phase'] == 'predict' and cfg['predict_set'] == 'val' and cfg['predict_stride'] == 16 and cfg['predict_flip'] is True
    assert t3.load_config3d(None, {'phase': 'train'})['phase'] == 'train' and t3.load_config3d(None, {'phase': 'test'})['phase'] == 'test'
    path, over = t3.parse_argv(['config3d.yaml', 'ckpt_path=/x', 'phase=predict', 'predict_stride=32'])
    assert path == 'config3d.yaml' and over['phase'] == 'predict' and t3.load_config3d(None, over)['predict_stride'] == 32
    with pytest.raises(KeyError):
        t3.load_config3d(None, {'predict_window': 3})             # unknown keys are still refused
    for bad in ({'phase': 'infer'}, {'predict_set': 'all'}, {'predict_stride': 0}):
        with pytest.raises(ValueError):
            t3.load_config3d(None, bad)


def test_example_config_lists_the_predict_keys(mrdis):
    with open(os.path.join(ROOT, 'config3d.yaml')) as f:
        y = yaml.safe_load(f)
    for k in ('predict_set', 'predict_stride', 'predict_flip'):
        assert k in y and y[k] == mrdis.train3d.DEFAULT_CONFIG_3D[k], k
    assert set(y) == set(mrdis.train3d.DEFAULT_CONFIG_3D)
    assert mrdis.train3d.load_config3d(os.path.join(ROOT, 'config3d.yaml'), {'phase': 'predict'})['phase'] == 'predict'


def test_binding_table_and_exports_know_the_new_entries(mrdis):
    for name in ('mrdis_seg_accum', 'mrdis_seg_label_volume'):
        assert name in mrdis.hip.EXPORTED_SYMBOLS
    assert mrdis.hip.SEGVOL_FAMILIES == ('segaccum', 'seglabels')
    lib = mrdis.hip.load()
    for fam in mrdis.hip.SEGVOL_FAMILIES:
        assert lib.mrdis_launch_count(fam.encode()) >= 0
    for name in ('predict_volumes', 'window_offsets', 'seg_metrics_from_counts'):
        assert hasattr(mrdis, name)
