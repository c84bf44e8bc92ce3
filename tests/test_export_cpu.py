"""Host half of the NIfTI export, no GPU: write_nifti against read_nifti, the geometry read_nifti now keeps, the new entry point in the header, the
library and the binding table, the configuration keys, and the float64 restatement of the kernel's rule (tests/export_check.py) on values worked
out by hand."""
import gzip
import os
import re
import struct

import numpy as np
import pytest
import yaml

import export_check as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRY = {'dim_info': 57, 'xyzt_units': 10, 'pixdim': (-1.0, 1.0, 1.25, 0.5, 2.0, 0.0, 0.0, 0.0), 'qform_code': 1, 'sform_code': 2,
            'quatern_b': 0.0, 'quatern_c': 1.0, 'quatern_d': 0.0, 'qoffset_x': 0.0, 'qoffset_y': -239.0, 'qoffset_z': 0.5,
            'srow_x': (-1.0, 0.0, 0.0, 0.0), 'srow_y': (0.0, -1.25, 0.0, 239.0), 'srow_z': (0.0, 0.0, 0.5, 0.25)}
KEYS_BEFORE = ('shape', 'datatype', 'slope', 'inter', 'pixdim', 'byteswapped')


@pytest.fixture(scope='module')
def m():
    import mrdis
    return mrdis


def voxels(kind, seed=0):
    """(D, W, H) = (3, 4, 5): file order of an (H, W, D) = (5, 4, 3) volume"""
    g = np.random.RandomState(seed)
    if kind == 'f4':
        return g.randn(3, 4, 5).astype(np.float32)
    info = np.iinfo(np.dtype(kind))
    return g.randint(info.min, info.max + 1, (3, 4, 5)).astype(kind)


def source_header(e, geometry):
    """a 348 + 4 byte NIfTI-1 header of a (5, 4, 3) int16 volume in byte order `e`, carrying `geometry`, packed here field by field"""
    hdr = bytearray(352)
    struct.pack_into(e + 'i', hdr, 0, 348)
    hdr[39] = geometry['dim_info']
    struct.pack_into(e + '8h', hdr, 40, 3, 5, 4, 3, 1, 1, 1, 1)
    struct.pack_into(e + '2h', hdr, 70, 4, 16)
    struct.pack_into(e + '8f', hdr, 76, *geometry['pixdim'])
    struct.pack_into(e + '3f', hdr, 108, 352.0, 1.0, 0.0)
    hdr[123] = geometry['xyzt_units']
    struct.pack_into(e + '2h', hdr, 252, geometry['qform_code'], geometry['sform_code'])
    struct.pack_into(e + '6f', hdr, 256, *(geometry[k] for k in ('quatern_b', 'quatern_c', 'quatern_d', 'qoffset_x', 'qoffset_y', 'qoffset_z')))
    struct.pack_into(e + '12f', hdr, 280, *geometry['srow_x'], *geometry['srow_y'], *geometry['srow_z'])
    hdr[344:348] = b'n+1\0'
    return bytes(hdr)


@pytest.mark.parametrize('e', ['<', '>'])
def test_read_nifti_keeps_the_geometry_and_its_old_keys(m, tmp_path, e):
    a = voxels('i2', 1)
    path = tmp_path / 'src.nii'
    path.write_bytes(source_header(e, GEOMETRY) + a.astype(np.dtype(e + 'i2')).tobytes())
    raw, info = m.read_nifti(str(path))
    assert np.array_equal(raw, a)
    assert info['geometry'] == GEOMETRY
    assert tuple(info)[:6] == KEYS_BEFORE and set(info) == set(KEYS_BEFORE) | {'geometry'}
    assert info['shape'] == (5, 4, 3) and info['datatype'] == 4 and (info['slope'], info['inter']) == (1.0, 0.0)
    assert info['pixdim'] == (1.0, 1.25, 0.5) and info['byteswapped'] == (e != ('<' if np.little_endian else '>'))


@pytest.mark.parametrize('ext', ['.nii', '.nii.gz'])
@pytest.mark.parametrize('kind,code', [('u1', 2), ('i2', 4), ('f4', 16)])
@pytest.mark.parametrize('source', [None, '<', '>'])
def test_write_nifti_round_trip(m, tmp_path, kind, code, ext, source):
    """the voxels, shape, datatype, slope 1 / inter 0 and every geometry field come back; the geometry is one parsed from a source file of either byte
    order, or none"""
    geometry = None
    if source:
        (tmp_path / 'src.nii').write_bytes(source_header(source, GEOMETRY) + voxels('i2').astype(np.dtype(source + 'i2')).tobytes())
        geometry = m.read_nifti(str(tmp_path / 'src.nii'))[1]['geometry']
        assert geometry == GEOMETRY
    v = voxels(kind, code)
    path = str(tmp_path / ('out' + ext))
    assert m.write_nifti(path, v, geometry) == path
    raw, info = m.read_nifti(path)
    assert raw.dtype == v.dtype and raw.shape == (3, 4, 5) and np.array_equal(raw.view(np.uint8), v.view(np.uint8))
    assert info['shape'] == (5, 4, 3) and info['datatype'] == code and info['slope'] == 1.0 and info['inter'] == 0.0
    assert info['byteswapped'] == (not np.little_endian)
    assert info['geometry'] == (GEOMETRY if source else m.prep.DEFAULT_GEOMETRY)
    if not source:
        g = info['geometry']
        assert g['pixdim'] == (1.0,) * 8 and g['qform_code'] == 0 and g['sform_code'] == 0


def test_header_bytes_and_reproducible_gz(m, tmp_path):
    v = voxels('i2', 3)
    a, b, plain = str(tmp_path / 'a.nii.gz'), str(tmp_path / 'sub_b.nii.gz'), str(tmp_path / 'p.nii')
    m.write_nifti(a, v, GEOMETRY)
    m.write_nifti(b, v, GEOMETRY)
    m.write_nifti(plain, v, GEOMETRY, descrip=b'x' * 79)
    assert open(a, 'rb').read() == open(b, 'rb').read()                          # no file name, no time stamp
    blob = open(plain, 'rb').read()
    assert gzip.open(a, 'rb').read()[:148] == blob[:148] and len(blob) == 352 + v.nbytes
    assert struct.unpack_from('<i', blob, 0)[0] == 348 and struct.unpack_from('<f', blob, 108)[0] == 352.0
    assert struct.unpack_from('<8h', blob, 40) == (3, 5, 4, 3, 1, 1, 1, 1) and struct.unpack_from('<2h', blob, 70) == (4, 16)
    assert struct.unpack_from('<2f', blob, 112) == (1.0, 0.0)
    assert blob[148:228] == b'x' * 79 + b'\0' and blob[344:348] == b'n+1\0' and blob[348:352] == b'\0\0\0\0'
    assert blob[352:] == v.astype('<i2').tobytes()
    assert gzip.open(a, 'rb').read()[148:153] == b'mrdis'


def test_write_nifti_refusals_name_the_argument(m, tmp_path):
    p = str(tmp_path / 'x.nii')
    v = voxels('i2')
    for bad, name in ((v[0], 'voxels'), (v.astype(np.int64), 'voxels'), (v.astype(np.float16), 'voxels'), (v.transpose(2, 1, 0), 'voxels'),
                      (v[:, :, ::2], 'voxels'), (v.tolist(), 'voxels')):
        with pytest.raises(ValueError, match=name):
            m.write_nifti(p, bad)
    with pytest.raises(ValueError, match='descrip'):
        m.write_nifti(p, v, descrip=b'y' * 80)
    with pytest.raises(ValueError, match='geometry'):
        m.write_nifti(p, v, geometry={'pixdim': (1.0, 1.0, 1.0)})
    with pytest.raises(ValueError, match='geometry'):
        m.write_nifti(p, v, geometry={'affine': None})
    assert not os.path.exists(p)


def test_entry_point_is_declared_exported_and_counted(m):
    hdr = open(os.path.join(ROOT, 'include', 'mrdis.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'\bint\s+mrdis_export_volume\s*\(', code)
    for name, value in (('MRDIS_EXPORT_COPY', 0), ('MRDIS_EXPORT_UNZSCORE', 1), ('MRDIS_EXPORT_UNMEAN', 2)):
        assert re.search(rf'#define\s+{name}\s+{value}\b', code)
    hip = m.hip
    lib = hip.load()
    assert 'mrdis_export_volume' in hip.EXPORTED_SYMBOLS and hasattr(lib, 'mrdis_export_volume')
    assert hip.EXPORT_FAMILIES == ('export',) and hip.EXPORT_KINDS == ('copy', 'unzscore', 'unmean')
    others = [v for k, v in vars(hip).items() if k.endswith('_FAMILIES') and k != 'EXPORT_FAMILIES']
    assert len(others) >= 14 and not any(set(hip.EXPORT_FAMILIES) & set(t) for t in others)
    assert lib.mrdis_launch_count(b'export') == hip.launch_counts()['export'] >= 0
    assert len(hip.OPTION_NAMES) == 28 and len(hip.ELEM_FAMILIES) == 12
    assert 'mrdis_export.hip' in open(os.path.join(ROOT, 'representation-disentanglement_amd', 'csrc', 'Makefile')).read()


def test_config_keys(m):
    t3 = m.train3d
    assert t3.DEFAULT_CONFIG_3D['write_nifti'] is False
    y = yaml.safe_load(open(os.path.join(ROOT, 'config3d.yaml')))
    assert y == t3.DEFAULT_CONFIG_3D
    with pytest.raises(ValueError, match='write_nifti'):
        t3.load_config3d(None, {'write_nifti': True, 'data_source': 'h5'})
    with pytest.raises(ValueError, match='write_nifti'):
        t3.load_config3d(None, {'write_nifti': 'yes', 'data_source': 'raw', 'raw_path': '/x'})
    assert t3.load_config3d(None, {'write_nifti': True, 'data_source': 'raw', 'raw_path': '/x'})['write_nifti'] is True
    assert m.DEFAULT_CONFIG['write_nifti'] is False and m.DEFAULT_CONFIG['synth_units'] == 'store'
    assert m.train.EXPORT_KEYS == ('write_nifti', 'synth_units') and m.train.SYNTH_UNITS == ('store', 'scan')


def test_export_keys_come_from_the_current_file(m, tmp_path, monkeypatch):
    """like phase and the seg_* / synth_* keys: a config.yaml saved under ckpt_path does not bring write_nifti or synth_units back"""
    seen = {}

    class FakeRun:
        rank = 0

        def __init__(self, config):
            seen['config'] = config

        def evaluate(self, **kw):
            return {}

        def synthesize(self, **kw):
            return {}
    monkeypatch.setattr(m.train, 'Run', FakeRun)
    base = {'ckpt_root': str(tmp_path / 'ckpt'), 'ckpt_timelabel': 'run0'}
    p = tmp_path / 'config.yaml'
    p.write_text(yaml.dump({**base, 'phase': 'test', 'write_nifti': True, 'synth_units': 'scan'}))
    m.train.main([str(p)])                                                  # leaves config.yaml with both keys set behind
    saved = yaml.safe_load(open(os.path.join(seen['config']['ckpt_path'], 'config.yaml')))
    assert saved['write_nifti'] is True and saved['synth_units'] == 'scan'
    p.write_text(yaml.dump({**base, 'phase': 'synthesize'}))
    m.train.main([str(p)])
    cfg = seen['config']
    assert cfg['phase'] == 'synthesize' and cfg['write_nifti'] is False and cfg['synth_units'] == 'store'
    p.write_text(yaml.dump({**base, 'phase': 'synthesize', 'write_nifti': True, 'synth_units': 'scan'}))
    m.train.main([str(p)])
    assert seen['config']['write_nifti'] is True and seen['config']['synth_units'] == 'scan'


def test_stores_without_raw_meta_are_refused(m):
    import torch
    for store in (m.VolumeStore(torch.device('cpu')), m.VolumeStore3D(torch.device('cpu')),
                  m.VolumeStore.from_arrays({'S/T1': np.zeros((4, 4, 2), np.float32)}, torch.device('cpu'))):
        assert store.raw_meta is None
        with pytest.raises(ValueError, match='data_source raw'):
            m.save_nifti('x.nii.gz', torch.zeros((4, 4, 2), dtype=torch.uint8), store, 'S')
    with pytest.raises(ValueError, match='data_source raw'):
        m.export_store_volume(store, 'S/T1', 'x.nii.gz')
    run = m.train.Run.__new__(m.train.Run)
    run.config = {'write_nifti': True}
    with pytest.raises(ValueError, match='data_source raw'):
        run._nifti_options(store)
    run.config = {'write_nifti': False}
    assert run._nifti_options(store) is False


# ---------------------------------------------------------------------------------------------- the float64 restatement, by hand
def test_conversion_ties_saturation_nan():
    inf = float('inf')
    y = [0.5, 1.5, 2.5, -0.5, 40000.0, -40000.0, 300.0, -1.0, float('nan'), inf, -inf, 254.5, 255.5, -32768.5]
    assert X.convert(y, 'i2').tolist() == [0, 2, 2, 0, 32767, -32768, 300, -1, 0, 32767, -32768, 254, 256, -32768]
    assert X.convert(y, 'u1').tolist() == [0, 2, 2, 0, 255, 0, 255, 0, 0, 255, 0, 254, 255, 0]
    f = X.convert(y, 'f4')
    assert f.dtype == np.float32 and np.isnan(f[8]) and f[9] == inf and f[10] == -inf and f[0] == 0.5 and f[4] == 40000.0
    assert X.convert([0.1], 'f4')[0] == np.float32(0.1) and X.convert([1e300], 'f4')[0] == inf


def test_rule_on_hand_written_values():
    # n = 3, sum = 8, ssd = 16: norm = 8 / 4 = 2, std = sqrt(16 / 4) = 2
    stats = np.array([[3.0, 8.0, 16.0, 9.0, 0.0]])
    src = np.array([-10.0, 0.0, 1.0, -0.5, 0.25], dtype=np.float32).reshape(1, 5, 1, 1)       # (B, H', W', D)
    got, y = X.export(src, ((1, 2), (0, 1)), 'hwd', 'unzscore', stats, 7.0, np.int16)
    assert got.shape == (1, 1, 2, 8) and y.shape == got.shape
    assert y[0, 0, 0].tolist() == [7.0, 0.0, 2.0, 1.0 * (2.0 + 1e-8) + 2.0, -0.5 * (2.0 + 1e-8) + 2.0, 0.25 * (2.0 + 1e-8) + 2.0, 7.0, 7.0]
    assert got[0, 0, 0].tolist() == [7, 0, 2, 4, 1, 3, 7, 7] and (got[0, 0, 1] == 7).all()
    got, y = X.export(src, ((0, 0), (0, 0)), 'hwd', 'unmean', stats, 0.0, np.float32)
    assert got[0, 0, 0].tolist() == [-20.0, 0.0, 2.0, -1.0, 0.5]
    lab = np.arange(24, dtype=np.uint8).reshape(1, 2, 3, 4)                                    # (B, D, H', W') for 'dhw'
    got, _ = X.export(lab, ((0, 1), (1, 0)), 'dhw', 'copy', None, 9.0, np.uint8)
    assert got.shape == (1, 2, 5, 4) and (got[:, :, 0] == 9).all() and (got[:, :, :, 3] == 9).all()
    assert np.array_equal(got[0, :, 1:, :3], lab[0].transpose(0, 2, 1))
    hwd = np.ascontiguousarray(lab.transpose(0, 2, 3, 1))                                      # the same volume as (B, H', W', D)
    assert np.array_equal(X.export(hwd, ((0, 1), (1, 0)), 'hwd', 'copy', None, 9.0, np.uint8)[0], got)
    assert X.tie_margin([0.5, 3.0]) == 0.0 and X.tie_margin([0.25, 7.0, float('nan')]) == 0.25
