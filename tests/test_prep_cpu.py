"""Host half of prep.py, no GPU: the NIfTI-1 reader on files packed here with struct, the fold lists against the slicing rule restated in plain
numpy, the three new entry points in the binding table, and the 3-D example configuration."""
import gzip
import os
import struct

import numpy as np
import pytest
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP_KIND = {2: 'u1', 4: 'i2', 8: 'i4', 16: 'f4', 64: 'f8', 512: 'u2'}


@pytest.fixture(scope='module')
def m():
    import mrdis
    return mrdis


def pack_nifti(arr_hwd, code, e='<', vox_offset=352, slope=1.0, inter=0.0, ndim=3, dim4=1, magic=b'n+1\0', sizeof_hdr=348, pixdim=(1.0, 2.0, 3.0)):
    """bytes of a single-file NIfTI-1 holding arr_hwd (H, W, D): the first axis is the fastest in the file"""
    H, W, D = arr_hwd.shape
    hdr = bytearray(348)
    struct.pack_into(e + 'i', hdr, 0, sizeof_hdr)
    struct.pack_into(e + '8h', hdr, 40, ndim, H, W, D, dim4, 1, 1, 1)
    struct.pack_into(e + '2h', hdr, 70, code, 8 * np.dtype(NP_KIND.get(code, 'u1')).itemsize)
    struct.pack_into(e + '8f', hdr, 76, 1.0, *pixdim, 0.0, 0.0, 0.0, 0.0)
    struct.pack_into(e + '3f', hdr, 108, float(vox_offset), slope, inter)
    hdr[344:348] = magic
    data = np.asarray(arr_hwd).astype(np.dtype(e + NP_KIND.get(code, 'u1'))).transpose(2, 1, 0).tobytes()
    return bytes(hdr) + b'\0' * (int(vox_offset) - 348) + data


def volume(code, shape=(5, 4, 3), seed=0):
    g = np.random.RandomState(seed)
    kind = np.dtype(NP_KIND[code])
    if kind.kind == 'f':
        return g.randn(*shape).astype(kind)
    info = np.iinfo(kind)
    return g.randint(max(info.min, -30000), min(info.max, 60000), shape).astype(kind)


def write(path, blob):
    with (gzip.open(path, 'wb') if str(path).endswith('.gz') else open(path, 'wb')) as f:
        f.write(blob)
    return str(path)


@pytest.mark.parametrize('code', sorted(NP_KIND))
@pytest.mark.parametrize('e', ['<', '>'])
@pytest.mark.parametrize('ext,vox_offset', [('.nii', 352), ('.nii.gz', 416)])
def test_reader_round_trip(m, tmp_path, code, e, ext, vox_offset):
    a = volume(code, seed=code)
    raw, info = m.read_nifti(write(tmp_path / ('v' + ext), pack_nifti(a, code, e, vox_offset)))
    assert raw.shape == (3, 4, 5) and raw.flags.c_contiguous and raw.dtype == np.dtype(NP_KIND[code]) and raw.dtype.isnative
    assert np.array_equal(raw.transpose(2, 1, 0), a)
    assert info['shape'] == (5, 4, 3) and info['datatype'] == code and info['slope'] == 1.0 and info['inter'] == 0.0
    assert info['pixdim'] == (1.0, 2.0, 3.0)
    assert info['byteswapped'] == (e != ('<' if np.little_endian else '>'))


def test_reader_native_file_is_a_view_of_the_bytes_read(m, tmp_path):
    raw, _ = m.read_nifti(write(tmp_path / 'v.nii', pack_nifti(volume(4), 4, '<' if np.little_endian else '>')))
    assert raw.base is not None and not raw.flags.owndata


def test_reader_accepts_a_fourth_axis_of_one(m, tmp_path):
    a = volume(4, seed=3)
    raw, info = m.read_nifti(write(tmp_path / 'v.nii.gz', pack_nifti(a, 4, ndim=4, dim4=1)))
    assert info['shape'] == (5, 4, 3) and np.array_equal(raw.transpose(2, 1, 0), a)


@pytest.mark.parametrize('slope,inter,want', [(0.0, 7.0, (1.0, 0.0)), (float('nan'), 7.0, (1.0, 0.0)), (2.5, -3.0, (2.5, -3.0))])
def test_reader_scaling(m, tmp_path, slope, inter, want):
    a = volume(4, seed=4)
    raw, info = m.read_nifti(write(tmp_path / 'v.nii', pack_nifti(a, 4, slope=slope, inter=inter)))
    assert (info['slope'], info['inter']) == want
    assert np.array_equal(raw.transpose(2, 1, 0), a)                   # never scaled on the host


REFUSALS = [
    ('sizeof_hdr', dict(sizeof_hdr=540)),
    ('magic', dict(magic=b'ni1\0')),                                    # the two-file form
    ('magic', dict(magic=b'n+2\0')),
    ('datatype', dict(code=128)),                                       # RGB24
    ('datatype', dict(code=256)),                                       # int8
    ('dim', dict(ndim=4, dim4=2)),                                      # four non-singleton axes
    ('dim', dict(ndim=5)),
    ('dim', dict(ndim=2)),
    ('vox_offset', dict(vox_offset=348)),
    ('vox_offset', dict(vox_offset=0)),
]


@pytest.mark.parametrize('field,kw', REFUSALS)
def test_reader_refuses_and_names_the_field(m, tmp_path, field, kw):
    kw = dict(kw)
    code = kw.pop('code', 4)
    blob = pack_nifti(volume(4), code, **{**kw, 'vox_offset': max(352, kw.get('vox_offset', 352))})
    if 'vox_offset' in kw:                                              # the header states the refused offset; the bytes stay where they are
        blob = blob[:108] + struct.pack('<f', float(kw['vox_offset'])) + blob[112:]
    with pytest.raises(ValueError, match=field):
        m.read_nifti(write(tmp_path / 'v.nii', blob))


def test_reader_refuses_truncated_files(m, tmp_path):
    blob = pack_nifti(volume(4), 4)
    with pytest.raises(ValueError, match='dim'):                        # voxels missing
        m.read_nifti(write(tmp_path / 'a.nii', blob[:-2]))
    with pytest.raises(ValueError, match='dim'):
        m.read_nifti(write(tmp_path / 'a.nii.gz', blob[:400]))
    with pytest.raises(ValueError, match='sizeof_hdr'):                 # not even a header
        m.read_nifti(write(tmp_path / 'b.nii', blob[:100]))


def expected_lists(ids, slices):
    """data_preprocessing_BraTS.py:100-146 in plain numpy: {file name: text}"""
    ids = list(ids)
    np.random.RandomState(10).shuffle(ids)
    n = len(ids)
    k = int(0.2 * n)
    out = {}
    for f in range(5):
        test = ids[f * k:(f + 1) * k]
        tv = ids[:f * k] + ids[(f + 1) * k:]
        val, train = tv[:int(0.1 * len(tv))], tv[int(0.1 * len(tv)):]
        for name, part in (('train', train), ('val', val), ('test', test)):
            part = [s for s in part if 'Validation' not in s]
            out[f'fold_BraTS_{f}_{name}_noval.txt'] = ''.join(f'{s} {i}\n' for s in part for i in range(*slices))
            out[f'fold_BraTS_3d_{f}_{name}_noval.txt'] = ''.join(s + '\n' for s in part)
    return out


@pytest.mark.parametrize('n,slices', [(13, (50, 105)), (40, (3, 12))])
def test_fold_lists(m, tmp_path, n, slices):
    ids = [f'BraTS20_Training_{i:03d}' for i in range(n - 3)] + [f'BraTS20_Validation_{i:03d}' for i in range(3)]
    np.random.seed(123)
    state = np.random.get_state()
    paths = m.write_fold_lists(ids, str(tmp_path), slices=slices)
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]      # the global stream is untouched
    want = expected_lists(ids, slices)
    assert sorted(os.path.basename(p) for p in paths) == sorted(want) == sorted(os.listdir(tmp_path))
    for name, text in want.items():
        assert open(tmp_path / name).read() == text, name
    # the same permutation as the reference's np.random.seed(10); np.random.shuffle
    np.random.seed(10)
    legacy = list(ids)
    np.random.shuffle(legacy)
    mine = list(ids)
    np.random.RandomState(10).shuffle(mine)
    assert legacy == mine
    tests = [set(want[f'fold_BraTS_3d_{f}_test_noval.txt'].split()) for f in range(5)]
    assert all(tests) and sum(len(t) for t in tests) == len(set().union(*tests))                        # disjoint
    assert not any('Validation' in text for text in want.values())
    for f in range(5):
        for name in ('train', 'val', 'test'):
            ids3 = want[f'fold_BraTS_3d_{f}_{name}_noval.txt'].split()
            if ids3:
                subj, idx = m.load_idx_list(str(tmp_path / f'fold_BraTS_{f}_{name}_noval.txt'))
                assert list(subj) == [s for s in ids3 for _ in range(*slices)] and list(idx) == list(range(*slices)) * len(ids3)
            if len(ids3) > 1:                                           # the 3-D reader takes the first line as a header (data3d.load_subj_list)
                assert list(m.load_subj_list(str(tmp_path / f'fold_BraTS_3d_{f}_{name}_noval.txt'))) == ids3[1:]


def test_abi_of_the_prep_entry_points(m):
    hip = m.hip
    lib = hip.load()
    for name in ('mrdis_prep_stats', 'mrdis_prep_write', 'mrdis_prep_workspace'):
        assert name in hip.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert hip.PREP_FAMILIES == ('prepstats', 'prepwrite')
    assert set(hip.PREP_FAMILIES) <= set(hip.launch_counts())
    for fam in hip.PREP_FAMILIES:
        assert lib.mrdis_launch_count(fam.encode()) >= 0
    assert len(hip.OPTION_NAMES) == 28 and len(hip.ELEM_FAMILIES) == 12
    assert lib.mrdis_prep_workspace(240, 240, 155) > 0
    assert lib.mrdis_prep_workspace(1025, 8, 8) == 0 and lib.mrdis_prep_workspace(0, 8, 8) == 0 and lib.mrdis_prep_workspace(1024, 1024, 1024) > 0
    # refused before any launch, on the host: no device is touched
    before = hip.launch_counts()
    assert lib.mrdis_prep_stats(1 << 12, 4, 1, 8, 64, 8, 8, 2048, 0, 0, 0, 0, 0, 0, 1.0, 0.0, 1 << 12, 1 << 12, 1 << 20, None) == -2
    assert lib.mrdis_prep_stats(1 << 12, 4, 1, 8, 64, 8, 8, 8, 4, 4, 0, 0, 0, 0, 1.0, 0.0, 1 << 12, 1 << 12, 1 << 20, None) == -2       # empty crop
    assert lib.mrdis_prep_stats(1 << 12, 32, 1, 8, 64, 8, 8, 8, 0, 0, 0, 0, 0, 0, 1.0, 0.0, 1 << 12, 1 << 12, 1 << 20, None) == -1      # complex64
    assert lib.mrdis_prep_write(1 << 12, 4, 1, 8, 64, 8, 8, 8, 0, 0, 0, 8, 1.0, 0.0, 1 << 12, 0, 0, 1 << 12, None) == -2
    assert lib.mrdis_prep_write(1 << 12, 4, 1, 8, 64, 8, 8, 8, 0, 0, 0, 0, 1.0, 0.0, 1 << 12, 3, 0, 1 << 12, None) == -1                # no such kind
    assert hip.launch_counts() == before


def test_config3d_yaml_states_the_defaults(m):
    t3 = m.train3d
    with open(os.path.join(ROOT, 'config3d.yaml')) as f:
        y = yaml.safe_load(f)
    assert y == t3.DEFAULT_CONFIG_3D
    assert y['data_source'] == 'h5' and y['raw_path'] == ''
    assert t3.load_config3d(None, {'data_source': 'raw', 'raw_path': '/x'})['raw_path'] == '/x'
    with pytest.raises(ValueError, match='raw_path'):
        t3.load_config3d(None, {'data_source': 'raw'})
    with pytest.raises(ValueError, match='data_source'):
        t3.load_config3d(None, {'data_source': 'nifti'})
