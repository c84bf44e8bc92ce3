"""mrdis_export_volume (csrc/mrdis_export.hip), hip.export_volume, save_nifti / export_store_volume and the write_nifti switches of the entry points,
against the float64 restatement of the rule in tests/export_check.py.

Bounds.  Integer destinations are compared EXACTLY: the inputs are built so that the fractional part of the float64 reference is at least 1e-6 away
from 0.5 on every voxel (asserted on the reference before comparing: a condition on the input, not a tolerance; the device's norm and std may
differ from numpy's in the last float64 bit, about 1e-13 of a value below 1e5).  float32 destinations are within 1 fp32 ulp of the float64 result
rounded to fp32, the bound tests/test_gpu_prep.py holds prep_write to, for the same reason; COPY and the fill margin match to the bit.
Round trip: z = fp32((v - norm) / den) is off by at most 2^-24 |z|, so z den + norm is off by at most 2^-24 |v - norm| < 0.004 for int16 voxels:
rounding gives v back exactly; v <= 0 became -10 and comes back as 0.  The mean rule destroys nothing, so v / norm comes back as v for EVERY voxel,
which is max(v, 0) wherever v >= 0 (checked both ways).
Shapes (H', W', D) with crop: (1, 1, 1); (5, 4, 3); (65, 66, 7) with H = 68 and h0 odd, every extent one past a 64 tile; (64, 64, 64); (130, 3, 67)
with H = 131, so rows of a narrow destination are never 4-byte aligned; B = 3 with statistics per volume; `out=` a view at an odd offset."""
import os
import shutil

import numpy as np
import pytest
import torch
import yaml

import export_check as X

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
NO_CROP = ((0, 0), (0, 0))
# (H', W', D), crop, B, element offset of `out` in a larger buffer (0: the binding allocates)
CASES = [((1, 1, 1), NO_CROP, 1, 0), ((5, 4, 3), ((1, 2), (0, 3)), 1, 0), ((65, 66, 7), ((3, 0), (0, 1)), 1, 0), ((64, 64, 64), NO_CROP, 1, 0),
         ((130, 3, 67), ((0, 1), (2, 0)), 1, 0), ((9, 6, 5), ((2, 1), (1, 0)), 3, 0), ((65, 66, 7), ((3, 0), (0, 1)), 1, 3)]
COMBOS = [('u1', 'copy', d) for d in ('u1', 'i2', 'f4')] + [('f4', k, d) for k in ('copy', 'unzscore', 'unmean') for d in ('u1', 'i2', 'f4')]
TORCH = {'u1': torch.uint8, 'i2': torch.int16, 'f4': torch.float32}
FILL = {'copy': -3.0, 'unzscore': 0.0, 'unmean': 7.0}
MARGIN = 1e-6


def stats_rows(B, kind):
    """(B, 5) float64 in the layout of mrdis_prep_stats, different per volume; norm and std are no round numbers"""
    n = np.array([1000.0 + 37 * b for b in range(B)])
    norm = np.array([500.3 + 11.7 * b for b in range(B)]) if kind == 'unzscore' else np.array([173.9 + 5.3 * b for b in range(B)])
    std = np.array([310.7 + 3.1 * b for b in range(B)])
    return np.stack([n, norm * (n + 1.0), std * std * (n + 1.0), np.full(B, 9.0), np.zeros(B)], 1)


def make_source(shape, B, src_kind, kind, seed):
    """(B, H', W', D): uint8 labels, or float32 values whose image under `kind` keeps clear of the rounding ties (those that do not are replaced by
    the background value, whose image is 0)"""
    g = np.random.RandomState(seed)
    full = (B,) + tuple(shape)
    if src_kind == 'u1':
        return g.randint(0, 256, full).astype(np.uint8)
    if kind == 'copy':
        s = (g.randint(-320000, 320000, full) / 8.0).astype(np.float32)       # eighths up to +-40000: both integer types saturate somewhere
        s[np.abs(s - np.floor(s)) == 0.5] += np.float32(0.25)
        return s
    s = (g.randn(*full) * (1.5 if kind == 'unzscore' else 2.0)).astype(np.float32)
    s[g.rand(*full) < 0.2] = np.float32(-10.0)
    y = X.values(s, NO_CROP, 'hwd', kind, stats_rows(B, kind))
    near = np.abs(np.abs(y - np.floor(y)) - 0.5) < 10 * MARGIN
    s[near.transpose(0, 3, 2, 1)] = np.float32(-10.0 if kind == 'unzscore' else 0.0)
    return s


def ulp_ok(got, want64):
    want = X.convert(want64, 'f4')
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)


@pytest.mark.parametrize('layout', ['hwd', 'dhw'])
@pytest.mark.parametrize('case', range(len(CASES)))
def test_table_against_float64(mrdis, case, layout):
    shape, crop, B, off = CASES[case]
    (h0, h1), (w0, w1) = crop
    Hc, Wc, D = shape
    H, W = Hc + h0 + h1, Wc + w0 + w1
    for k, (src_kind, kind, dst_kind) in enumerate(COMBOS):
        what = (shape, crop, B, layout, src_kind, kind, dst_kind)
        src = make_source(shape, B, src_kind, kind, seed=100 * case + k)
        lay = src if layout == 'hwd' else np.ascontiguousarray(src.transpose(0, 3, 1, 2))
        stats = None if kind == 'copy' else stats_rows(B, kind)
        want, y = X.export(lay, crop, layout, kind, stats, FILL[kind], np.dtype(dst_kind))
        assert want.shape == (B, D, W, H)
        t = torch.from_numpy(lay).to(DEV)
        if B == 1:
            t = t[0]
        st = None if stats is None else torch.from_numpy(stats if B > 1 else stats[0]).to(DEV)
        out = None
        if off:
            buf = torch.full((B * D * W * H + 2 * off + 5,), 77, dtype=TORCH[dst_kind], device=DEV)
            out = buf[off:off + D * W * H].view(D, W, H)
            assert out.data_ptr() % 4 != 0 or dst_kind == 'f4'
        got = mrdis.hip.export_volume(t, crop, layout, kind, st, FILL[kind], TORCH[dst_kind], out=out)
        assert got.dtype == TORCH[dst_kind] and got.is_contiguous() and tuple(got.shape) == ((B, D, W, H) if B > 1 else (D, W, H))
        if off:
            assert got is out
            rest = torch.cat([buf[:off], buf[off + D * W * H:]])
            assert bool((rest == 77).all()), what                              # nothing outside the view is touched
        got = got.cpu().numpy().reshape(B, D, W, H)
        if dst_kind != 'f4':
            assert X.tie_margin(y) >= MARGIN, what                             # the condition on the input
            assert np.array_equal(got, want), (what, int((got != want).sum()))
            continue
        inside = np.zeros((B, D, W, H), dtype=bool)
        inside[:, :, w0:w0 + Wc, h0:h0 + Hc] = True
        assert np.array_equal(got[~inside].view(np.int32), want[~inside].view(np.int32)), what            # the fill margin: to the bit
        if kind == 'copy':
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), what
        else:
            ok = ulp_ok(got, y)
            assert ok.all(), (what, int((~ok).sum()))
            zero = (lay == np.float32(-10.0)) if kind == 'unzscore' else np.zeros(lay.shape, bool)
            zero = zero.transpose(0, 3, 2, 1) if layout == 'hwd' else zero.transpose(0, 1, 3, 2)
            assert (got[:, :, w0:w0 + Wc, h0:h0 + Hc][zero] == 0.0).all(), what


def test_ties_saturation_and_nan_through_copy(mrdis):
    inf = float('inf')
    vals = [0.5, 1.5, 2.5, -0.5, 40000.0, -40000.0, 300.0, -1.0, float('nan'), inf, -inf, 254.5, 255.5, -32768.5]
    src = torch.tensor(vals, dtype=torch.float32, device=DEV).view(len(vals), 1, 1)             # (H', W', D)
    want = {'i2': [0, 2, 2, 0, 32767, -32768, 300, -1, 0, 32767, -32768, 254, 256, -32768], 'u1': [0, 2, 2, 0, 255, 0, 255, 0, 0, 255, 0, 254, 255, 0]}
    for kind, w in want.items():
        got = mrdis.hip.export_volume(src, NO_CROP, 'hwd', 'copy', None, 0.0, TORCH[kind]).cpu().numpy().reshape(-1)
        assert got.tolist() == w == X.convert(vals, kind).tolist(), kind
    got = mrdis.hip.export_volume(src, NO_CROP, 'hwd', 'copy', None, 0.0, torch.float32).cpu().numpy().reshape(-1)
    assert np.array_equal(got.view(np.int32), np.array(vals, dtype=np.float32).view(np.int32))
    for fill, w in ((float('nan'), 0), (2.5, 2), (1e9, 32767), (-inf, -32768)):                  # the fill goes through the same conversion
        got = mrdis.hip.export_volume(src[:1], ((1, 0), (0, 0)), 'hwd', 'copy', None, fill, torch.int16).cpu().numpy().reshape(-1)
        assert got.tolist() == [w, 0], fill


def make_raw(shape, seed):
    """(H, W, D) int16 of the make_volume kind of tests/test_gpu_prep.py: negatives, zeros, an all-background plane, values up to 32767"""
    g = np.random.RandomState(seed)
    a = g.randint(-200, 32768, shape).astype(np.int16)
    a[g.rand(*shape) < 0.2] = 0
    a[:, :, 0] = 0
    a[-1, -1, -1] = 32767
    return a


@pytest.mark.parametrize('layout', ['hwd', 'dhw'])
@pytest.mark.parametrize('norm', ['zscore', 'mean'])
def test_round_trip_gives_the_scan_back(mrdis, norm, layout):
    shape, crop = (70, 67, 9), ((3, 2), (1, 4))
    (h0, h1), (w0, w1) = crop
    raw = make_raw(shape, seed=3)
    t = torch.from_numpy(np.ascontiguousarray(raw.transpose(2, 1, 0))).to(DEV)                   # file order (D, W, H)
    vol, stats = mrdis.prep_volume(t, norm, crop, layout)
    back = mrdis.hip.export_volume(vol, crop, layout, 'unzscore' if norm == 'zscore' else 'unmean', stats, 0.0, torch.int16)
    got = back.cpu().numpy().transpose(2, 1, 0)                                                  # (H, W, D)
    inner = raw[h0:shape[0] - h1, w0:shape[1] - w1]
    want = np.zeros(shape, dtype=np.int16)
    want[h0:shape[0] - h1, w0:shape[1] - w1] = np.maximum(inner, 0) if norm == 'zscore' else inner
    assert got.dtype == np.int16 and np.array_equal(got, want)
    pos = inner >= 0
    assert np.array_equal(got[h0:shape[0] - h1, w0:shape[1] - w1][pos], np.maximum(inner, 0)[pos]) and (inner < 0).any() and pos.sum() > inner.size // 2


def test_one_launch_per_call_and_equal_bits(mrdis):
    hip = mrdis.hip
    g = np.random.RandomState(5)
    crop = ((2, 1), (0, 3))
    for B in (1, 15):
        src = torch.from_numpy(g.randint(0, 5, (B, 21, 18, 6)).astype(np.uint8)).to(DEV)
        f = torch.from_numpy(g.randn(B, 21, 18, 6).astype(np.float32)).to(DEV)
        st = torch.from_numpy(stats_rows(B, 'unzscore')).to(DEV)
        for args in ((src, crop, 'hwd', 'copy', None, 0.0, torch.uint8), (f, crop, 'hwd', 'unzscore', st, 0.0, torch.int16),
                     (f, crop, 'hwd', 'unzscore', st[0], 0.0, torch.float32)):
            c0 = hip.launch_counts()
            a = hip.export_volume(*args)
            c1 = hip.launch_counts()
            assert {k: c1[k] - c0[k] for k in c0 if c1[k] != c0[k]} == {'export': 1, 'all': 1}, B      # one count, one kernel launch, no other family
            assert tuple(a.shape) == (B, 6, 21, 24) and torch.equal(a, hip.export_volume(*args))
    view = f.permute(0, 2, 1, 3)                                                                 # a non-contiguous source is copied
    assert torch.equal(hip.export_volume(view, crop, 'hwd', dtype=torch.float32), hip.export_volume(view.contiguous(), crop, 'hwd', dtype=torch.float32))


def test_refusals_raise_before_any_launch(mrdis):
    hip = mrdis.hip
    lib = hip.load()
    u8 = torch.zeros((4, 6, 8), dtype=torch.uint8, device=DEV)
    f4 = torch.zeros((4, 6, 8), dtype=torch.float32, device=DEV)
    st = torch.zeros(5, dtype=torch.float64, device=DEV)
    before, all0 = hip.launch_counts(), lib.mrdis_launch_count(b'all')
    bad = [dict(src=torch.zeros((1025, 1, 1), dtype=torch.uint8, device=DEV)), dict(src=torch.zeros((1, 1, 1025), dtype=torch.uint8, device=DEV)),
           dict(src=torch.zeros((1000, 1, 1), dtype=torch.uint8, device=DEV), crop=((20, 10), (0, 0))),
           dict(src=torch.zeros((1, 1000, 1), dtype=torch.uint8, device=DEV), crop=((0, 0), (0, 25))),
           dict(src=torch.zeros((0, 4, 6, 8), dtype=torch.uint8, device=DEV)), dict(src=torch.zeros((65536, 1, 1, 1), dtype=torch.uint8, device=DEV)),
           dict(crop=((-1, 0), (0, 0))), dict(crop=((0, 0), (0, -2))), dict(layout='whd'), dict(kind='label'), dict(dtype=torch.int32),
           dict(src=f4.double()), dict(kind='unzscore', stats=st), dict(kind='unmean', stats=st),
           dict(src=f4, kind='unzscore', stats=None), dict(src=f4, kind='unmean', stats=None)]
    for kw in bad:
        args = dict(src=u8, crop=NO_CROP, layout='hwd', kind='copy', stats=None, fill=0.0, dtype=torch.uint8)
        args.update(kw)
        with pytest.raises(mrdis.MrdisError, match='unsupported geometry'):
            hip.export_volume(**args)
    with pytest.raises(mrdis.MrdisError, match='out must be'):
        hip.export_volume(u8, NO_CROP, 'hwd', out=torch.zeros((8, 6, 4), dtype=torch.int16, device=DEV))
    with pytest.raises(mrdis.MrdisError, match='stats must be'):
        hip.export_volume(f4, NO_CROP, 'hwd', 'unmean', st[:4], dtype=torch.int16)
    # the checks are the entry point's own: the same refusals from the C call, with MRDIS_EUNSUPPORTED (-2)
    out = torch.zeros(4 * 6 * 8, dtype=torch.float32, device=DEV)
    ok = dict(src=u8.data_ptr(), sdt=2, layout=1, Hc=4, Wc=6, D=8, h0=0, h1=0, w0=0, w1=0, B=1, kind=0, stats=None, fill=0.0, dst=out.data_ptr(), ddt=2,
              stream=None)
    for kw in (dict(Hc=0), dict(D=1025), dict(Hc=1000, h0=25), dict(B=0), dict(B=65536), dict(w1=-1), dict(sdt=4), dict(ddt=8), dict(layout=2),
               dict(kind=3), dict(kind=-1), dict(kind=1), dict(sdt=16, src=f4.data_ptr(), kind=2)):
        assert lib.mrdis_export_volume(*dict(ok, **kw).values()) == -2, kw
    assert hip.launch_counts() == before and lib.mrdis_launch_count(b'all') == all0


# ---------------------------------------------------------------------------------------------- trees of NIfTI files, end to end
SUFFIX = {'T1': 't1', 'T1c': 't1ce', 'T2': 't2', 'T2_FLAIR': 'flair', 'seg': 'seg'}


def geometry_of(subject_index, key):
    """a geometry that names its file: the offsets hold the subject's number and the key's place"""
    k = list(SUFFIX).index(key)
    return {'dim_info': 0, 'xyzt_units': 10, 'pixdim': (-1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0), 'qform_code': 1, 'sform_code': 1,
            'quatern_b': 0.0, 'quatern_c': 0.0, 'quatern_d': 1.0, 'qoffset_x': float(subject_index), 'qoffset_y': 239.0, 'qoffset_z': float(k),
            'srow_x': (-1.0, 0.0, 0.0, float(subject_index)), 'srow_y': (0.0, -1.0, 0.0, 239.0), 'srow_z': (0.0, 0.0, 1.0, float(k))}


def write_tree(mrdis, root, n, shape, contrasts, seed, skip=()):
    """n subjects of int16 scans (positive inside an ellipse, a few negatives, 0 outside) and uint8 labels, written with write_nifti, each file with
    its own geometry; `skip`: (subject, key) files left out -> {subject/key: (H, W, D) array}, the subject ids"""
    g = np.random.RandomState(seed)
    H, W, D = shape
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    inside = (((yy - H / 2 + 0.5) / (0.42 * H)) ** 2 + ((xx - W / 2 + 0.5) / (0.40 * W)) ** 2) <= 1
    arrays, names = {}, [f'BraTS20_Training_{i:03d}' for i in range(n)]
    for i, subj in enumerate(names):
        os.makedirs(os.path.join(root, subj))
        for key in list(contrasts) + ['seg']:
            if (subj, key) in skip:
                continue
            if key == 'seg':
                a = (g.randint(0, 5, shape) * (g.rand(*shape) < 0.2)).astype(np.uint8)
                a[H // 2, W // 2, 0] = 4
            else:
                a = (g.randint(1, 3000, shape) * inside[:, :, None]).astype(np.int16)
                a[H // 2, W // 2, :] = -7
            ext = '.nii.gz' if i % 4 == 0 else '.nii'
            mrdis.write_nifti(os.path.join(root, subj, f'{subj}_{SUFFIX[key]}{ext}'), np.ascontiguousarray(a.transpose(2, 1, 0)), geometry_of(i, key))
            arrays[f'{subj}/{key}'] = a
    return arrays, names


def read_all(top, exts=('.npy', '.csv')):
    """{relative path: bytes} of the files under `top` with one of the extensions"""
    out = {}
    for d, _, files in os.walk(top):
        for fn in files:
            if fn.endswith(exts):
                with open(os.path.join(d, fn), 'rb') as f:
                    out[os.path.relpath(os.path.join(d, fn), top)] = f.read()
    return out


def check_label_file(mrdis, path, npy, crop, geometry):
    """a label file on the full canvas: uint8, the interior transposed equals the .npy, the margin is 0, the geometry is the wanted one"""
    (h0, h1), (w0, w1) = crop
    raw, info = mrdis.read_nifti(path)
    v = np.load(npy)
    Hc, Wc, D = v.shape
    assert raw.dtype == np.uint8 and info['datatype'] == 2 and info['shape'] == (Hc + h0 + h1, Wc + w0 + w1, D)
    vol = raw.transpose(2, 1, 0)
    assert np.array_equal(vol[h0:h0 + Hc, w0:w0 + Wc], v)
    margin = np.ones(vol.shape, bool)
    margin[h0:h0 + Hc, w0:w0 + Wc] = False
    assert (vol[margin] == 0).all() and margin.any()
    assert info['geometry'] == geometry and (info['slope'], info['inter']) == (1.0, 0.0)


CROP3D = ((3, 5), (4, 0))


@pytest.fixture(scope='module')
def world3d(mrdis, tmp_path_factory):
    """15 subjects of 40 x 36 x 123 files whose crop is the 32 x 32 x 123 the raw-file tests train on; an untrained NVNet3D saved as model_best"""
    top = tmp_path_factory.mktemp('export3d')
    root = str(top / 'raw')
    os.makedirs(root)
    arrays, names = write_tree(mrdis, root, 15, (40, 36, 123), ['T1', 'T2'], seed=6)
    cfg = dict(dataset_name='BraTS', data_path=str(top / 'lists'), data_source='raw', raw_path=root, raw_crop=[list(c) for c in CROP3D],
               contrast_list=['T1', 'T2'], batch_size=2, model_name='NVNet3D', init_channels=8, epochs=1, max_batches=1, predict_stride=16,
               ckpt_path=str(top / 'ckpt'), device='cuda:0')
    run = mrdis.Run3D(cfg, log=lambda *a: None)
    torch.save({'model': run.model.state_dict(), 'epoch': 0, 'monitor_metric': 0.0}, os.path.join(cfg['ckpt_path'], 'model_best.pth.tar'))
    return dict(cfg=cfg, store=run.data.store, arrays=arrays, names=names, top=top)


def test_run3d_predict_writes_nifti_beside_unchanged_files(mrdis, world3d):
    w = world3d
    hip = mrdis.hip
    store = w['store']
    assert store.raw_meta['crop'] == CROP3D and store.raw_meta['shape'] == (40, 36, 123) and store.shape == (32, 32, 123)
    dirs = {}
    for name in ('off', 'on'):
        dirs[name] = str(w['top'] / name)
        shutil.copytree(w['cfg']['ckpt_path'], dirs[name])
    base = dict(w['cfg'], phase='predict', predict_post=True, post_min_voxels=30)
    c0 = hip.launch_counts()
    mrdis.Run3D(dict(base, ckpt_path=dirs['off'], write_nifti=False), store=store, log=lambda *a: None).predict()
    c1 = hip.launch_counts()
    mrdis.Run3D(dict(base, ckpt_path=dirs['on'], write_nifti=True), store=store, log=lambda *a: None).predict()
    c2 = hip.launch_counts()
    off, on = read_all(os.path.join(dirs['off'], 'result_test')), read_all(os.path.join(dirs['on'], 'result_test'))
    assert off == on and len(off) == 2 * 2 + 2                                 # two subjects, raw and cleaned, predict.csv and postprocess.csv
    assert not read_all(dirs['off'], ('.nii.gz', '.nii')) and c1['export'] == c0['export']
    assert c2['export'] - c1['export'] == 4                                    # one per subject and directory
    assert {k: c2[k] - c1[k] for k in c0 if k not in ('export', 'all')} == {k: c1[k] - c0[k] for k in c0 if k not in ('export', 'all')}
    out = os.path.join(dirs['on'], 'result_test')
    subjects = [fn[:-len('_seg.npy')] for fn in sorted(os.listdir(out)) if fn.endswith('_seg.npy')]
    assert len(subjects) == 2
    for s in subjects:
        i = w['names'].index(s)
        for d in (out, os.path.join(out, 'post')):
            check_label_file(mrdis, os.path.join(d, f'{s}_seg.nii.gz'), os.path.join(d, f'{s}_seg.npy'), CROP3D, geometry_of(i, 'seg'))
    # phase postprocess writes the same post/ files, NIfTI included (two writes of one volume are the same bytes)
    want = read_all(os.path.join(out, 'post'), ('.nii.gz', '.npy', '.csv'))
    shutil.rmtree(os.path.join(out, 'post'))
    mrdis.Run3D(dict(base, phase='postprocess', ckpt_path=dirs['on'], write_nifti=True), store=store, log=lambda *a: None).postprocess()
    got = read_all(os.path.join(out, 'post'), ('.nii.gz', '.npy', '.csv'))
    assert {k: v for k, v in got.items() if 'regions' not in k} == want
    with pytest.raises(ValueError, match='write_nifti'):
        mrdis.Run3D(dict(base, data_source='h5', write_nifti=True), store=store, log=lambda *a: None)


def test_export_store_volume_3d_reproduces_the_scan(mrdis, world3d, tmp_path):
    w = world3d
    (h0, h1), (w0, w1) = CROP3D
    s = w['names'][4]
    c0 = mrdis.hip.launch_counts()['export']
    for key, dt in (('T2', np.int16), ('seg', np.uint8)):
        p = mrdis.export_store_volume(w['store'], f'{s}/{key}', str(tmp_path / f'{key}.nii.gz'))
        raw, info = mrdis.read_nifti(p)
        a = w['arrays'][f'{s}/{key}']
        want = np.zeros_like(a)
        want[h0:40 - h1, w0:36 - w1] = np.maximum(a[h0:40 - h1, w0:36 - w1], 0)
        assert raw.dtype == dt and np.array_equal(raw.transpose(2, 1, 0), want) and (a < 0).any() == (key != 'seg')
        assert info['geometry'] == geometry_of(4, key)
    assert mrdis.hip.launch_counts()['export'] == c0 + 2
    with pytest.raises(ValueError, match='not in the store'):
        mrdis.export_store_volume(w['store'], f'{s}/T1c', str(tmp_path / 'x.nii.gz'))


CROP2D = ((5, 3), (2, 4))
NAMES2D = ['T1', 'T1c', 'T2']


@pytest.fixture(scope='module')
def world2d(mrdis, tmp_path_factory):
    """13 subjects of 72 x 70 x 16 files whose crop is the 64 x 64 x 16 the raw-file tests train on; an untrained model with an output decoder"""
    top = tmp_path_factory.mktemp('export2d')
    root = str(top / 'raw')
    os.makedirs(root)
    arrays, names = write_tree(mrdis, root, 13, (72, 70, 16), NAMES2D, seed=4)
    base = dict(contrast_list=NAMES2D, input_height=64, input_width=64, batch_size=8, epochs=1, gpu='0', data_source='raw', raw_path=root,
                raw_slices=[3, 12], raw_crop=[list(c) for c in CROP2D], data_path=str(top / 'lists'), ckpt_root=str(top / 'ckpt'), ckpt_timelabel='t0',
                dataset_name='BraTS', lambda_recon_y_fused=1.0, out_num_ch=4)
    (top / 'train.yaml').write_text(yaml.dump(base))
    cfg = mrdis.train.setup_config(str(top / 'train.yaml'), device=DEV)
    run = mrdis.train.Run(cfg, log=lambda *a: None)
    return dict(run=run, arrays=arrays, names=names, top=top, out=os.path.join(cfg['ckpt_path'], 'result_test'))


def test_run_segment_writes_nifti_with_one_launch_per_subject(mrdis, world2d):
    w = world2d
    run, hip, out = w['run'], mrdis.hip, w['out']
    store = run.loaders['test'].dataset.store
    assert store.raw_meta['crop'] == CROP2D and store.raw_meta['norm_type'] == 'zscore' and store.shape == (64, 64, 16)
    run.config.update(write_nifti=False, seg_post=True, seg_post_min_voxels=20)
    shutil.rmtree(out, ignore_errors=True)                                     # whatever another test of this module left there
    c0 = hip.launch_counts()
    run.segment(patterns=[[], ['T1']])
    c1 = hip.launch_counts()
    off = read_all(out)
    assert not read_all(out, ('.nii.gz',)) and c1['export'] == c0['export']
    shutil.rmtree(out)
    run.config.update(write_nifti=True)
    run.segment(patterns=[[], ['T1']])
    c2 = hip.launch_counts()
    run.config.update(write_nifti=False, seg_post=False)
    assert read_all(out) == off
    subjects = sorted({fn[:-len('_seg.npy')] for fn in os.listdir(os.path.join(out, 'seg', 'full')) if fn.endswith('_seg.npy')})
    assert len(subjects) == 2 and c2['export'] - c1['export'] == 2             # one launch per subject: two patterns, raw and cleaned
    assert {k: c2[k] - c1[k] for k in c0 if k not in ('export', 'all')} == {k: c1[k] - c0[k] for k in c0 if k not in ('export', 'all')}
    for s in subjects:
        i = w['names'].index(s)
        for d in (os.path.join(out, 'seg'), os.path.join(out, 'seg', 'post')):
            for pat in ('full', 'no_T1'):
                check_label_file(mrdis, os.path.join(d, pat, f'{s}_seg.nii.gz'), os.path.join(d, pat, f'{s}_seg.npy'), CROP2D, geometry_of(i, 'seg'))


def test_run_synthesize_writes_store_and_scan_units(mrdis, world2d):
    w = world2d
    run, hip, out = w['run'], mrdis.hip, os.path.join(w['out'], 'synth')
    (h0, h1), (w0, w1) = CROP2D
    meta = run.loaders['test'].dataset.store.raw_meta
    c0 = hip.launch_counts()['export']
    shutil.rmtree(w['out'], ignore_errors=True)                               # whatever another test of this module left there
    run.config.update(write_nifti=False)
    run.synthesize(drop=['T2'])
    off = read_all(w['out'])
    assert hip.launch_counts()['export'] == c0 and not read_all(w['out'], ('.nii.gz',))
    files = sorted(fn for fn in os.listdir(out) if fn.endswith('.npy'))
    assert len(files) == 2 * 2                                                 # T1 and T1c of two subjects; the dropped T2 has no code without synth_info
    for units in ('store', 'scan'):
        shutil.rmtree(w['out'])
        run.config.update(write_nifti=True, synth_units=units)
        run.synthesize(drop=['T2'])
        run.config.update(write_nifti=False, synth_units='store')
        assert read_all(w['out']) == off
        for fn in files:
            s, c = fn[:-4].rsplit('_', 1)
            v = np.load(os.path.join(out, fn))
            raw, info = mrdis.read_nifti(os.path.join(out, fn[:-4] + '.nii.gz'))
            assert info['shape'] == (72, 70, 16) and info['geometry'] == geometry_of(w['names'].index(s), c)
            vol = raw.transpose(2, 1, 0)
            margin = np.ones(vol.shape, bool)
            margin[h0:72 - h1, w0:70 - w1] = False
            if units == 'store':
                assert raw.dtype == np.float32 and np.array_equal(vol[h0:72 - h1, w0:70 - w1].view(np.int32), v.view(np.int32))
                assert (vol[margin] == -10.0).all()
            else:
                want, y = X.export(v[None], CROP2D, 'hwd', 'unzscore', meta['subjects'][s][c]['stats_host'], 0.0, np.int16)
                clear = np.abs(np.abs(y - np.floor(y)) - 0.5) >= MARGIN
                assert raw.dtype == np.int16 and info['datatype'] == 4 and clear.mean() > 0.9999
                assert np.array_equal(raw[clear[0]], want[0][clear[0]]) and (vol[margin] == 0).all()
    assert hip.launch_counts()['export'] == c0 + 2 * 4
    run.config.update(write_nifti=True, synth_units='voxel')
    with pytest.raises(ValueError, match='synth_units'):
        run.synthesize(drop=['T2'])
    run.config.update(write_nifti=False, synth_units='store')


def test_export_store_volume_2d_and_the_fallback_for_a_contrast_without_a_file(mrdis, world2d, tmp_path):
    w = world2d
    (h0, h1), (w0, w1) = CROP2D
    store = w['run'].loaders['test'].dataset.store
    s = w['names'][7]
    p = mrdis.export_store_volume(store, f'{s}/T1c', str(tmp_path / 't1c.nii'))                  # the (D, H', W') layout's user
    raw, info = mrdis.read_nifti(p)
    a = w['arrays'][f'{s}/T1c']
    want = np.zeros_like(a)
    want[h0:72 - h1, w0:70 - w1] = np.maximum(a[h0:72 - h1, w0:70 - w1], 0)
    assert raw.dtype == np.int16 and np.array_equal(raw.transpose(2, 1, 0), want) and (a < 0).any() and info['geometry'] == geometry_of(7, 'T1c')
    # a subject without a T2 file and without a seg file: no statistics, so store units with one log line; geometry of its first file
    root = str(tmp_path / 'raw')
    os.makedirs(root)
    _, names = write_tree(mrdis, root, 1, (72, 70, 16), NAMES2D, seed=8, skip=(('BraTS20_Training_000', 'T2'), ('BraTS20_Training_000', 'seg')))
    lone, kept = mrdis.build_store_from_raw(root, DEV, store_cls=mrdis.VolumeStore3D, crop=CROP2D, log=lambda *a: None)
    assert kept == names and sorted(lone.raw_meta['subjects'][names[0]]) == ['T1', 'T1c']
    m0 = lone.raw_meta['subjects'][names[0]]['T1']
    assert set(m0) == {'stats', 'stats_host', 'geometry', 'datatype', 'slope', 'inter'} and m0['stats'].is_cuda and m0['datatype'] == 4
    assert np.array_equal(m0['stats'].cpu().numpy(), m0['stats_host'])
    vol = lone.vols[f'{names[0]}/T1']
    lines = []
    mrdis.save_nifti(str(tmp_path / 't2.nii.gz'), vol, lone, names[0], 'T2', units='scan', log=lines.append)
    assert len(lines) == 1 and 'T2' in lines[0] and 'store units' in lines[0]
    raw, info = mrdis.read_nifti(str(tmp_path / 't2.nii.gz'))
    got = raw.transpose(2, 1, 0)
    assert raw.dtype == np.float32 and np.array_equal(got[h0:72 - h1, w0:70 - w1].view(np.int32), vol.cpu().numpy().view(np.int32))
    assert (got[:h0] == -10.0).all() and (got[:, :w0] == -10.0).all() and info['geometry'] == geometry_of(0, 'T1')
    labels = torch.zeros((2, 64, 64, 16), dtype=torch.uint8, device=DEV)
    labels[1, 3, 4, 5] = 4
    mrdis.save_nifti([str(tmp_path / 'a.nii.gz'), str(tmp_path / 'b.nii.gz')], labels, lone, names[0], log=lines.append)
    raw, info = mrdis.read_nifti(str(tmp_path / 'b.nii.gz'))
    assert raw.dtype == np.uint8 and raw.sum() == 4 and raw[5, w0 + 4, h0 + 3] == 4 and info['geometry'] == geometry_of(0, 'T1') and len(lines) == 1
    for bad in (dict(path=[str(tmp_path / 'c.nii')], vol=labels), dict(vol=labels[0, :32]), dict(units='voxel'), dict(subj='nobody')):
        args = dict(path=str(tmp_path / 'c.nii'), vol=labels[0], store=lone, subj=names[0])
        args.update(bad)
        with pytest.raises(ValueError):
            mrdis.save_nifti(**args)
