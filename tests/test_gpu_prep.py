"""prep_stats / prep_write (csrc/mrdis_prep.hip) and build_store_from_raw against the float64 numpy statement of the rule
(data_preprocessing_BraTS.py:79-96), written here.

Bounds.  n, nan_inner and vmax are exact.  sum is exact for integer inputs with slope 1: every partial sum is an integer below 2^53.  Otherwise
sum and ssd are within a relative 1e-12 of numpy: both are fixed-order float64 sums of at most 2^23 terms (the float volumes here are positive
on average, as an MR scan is, so the sum does not cancel).  Every output voxel is within 1 fp32 ulp of the float64 result rounded to fp32: the
only difference allowed is the order of the sums behind norm and std, about 1e-13 relative against 6e-8 per ulp.  The -10 fill and label
volumes match to the bit.  Shapes: (37, 29, 11) with an odd crop, (70, 66, 65) -- one past a 64 tile on every axis, several workgroups of
partial sums --, (1, 1, 1), and (96, 80, 20) with a crop that is a multiple of nothing in particular and an empty inner range."""
import os
import struct

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
CASES = [((37, 29, 11), ((3, 2), (1, 4)), (2, 3)), ((70, 66, 65), ((0, 0), (0, 0)), (5, 7)), ((1, 1, 1), ((0, 0), (0, 0)), (0, 0)),
         ((96, 80, 20), ((16, 16), (8, 8)), (50, 50))]
DTYPES = ['u1', 'i2', 'u2', 'i4', 'f4', 'f8']
SCALES = {'u1': (1.0, 0.0), 'i2': (1.0, 0.0), 'u2': (2.5, -3.0), 'i4': (1.0, 0.0), 'f4': (1.0, 0.0), 'f8': (0.75, 0.125)}
KINDS = ('zscore', 'mean', 'label')


def make_volume(shape, kind, seed):
    """(H, W, D) with negatives, an all-background plane (d = 0) and, for the float kinds, NaNs inside and outside the inner planes"""
    g = np.random.RandomState(seed)
    H, W, D = shape
    dt = np.dtype(kind)
    if dt.kind == 'f':
        a = (g.randn(*shape) * 0.7 + 1.0).astype(dt)
        a[g.rand(*shape) < 0.02] = np.nan
    elif dt.kind == 'u':
        a = g.randint(0, min(np.iinfo(dt).max, 40000), shape).astype(dt)
        a[g.rand(*shape) < 0.3] = 0
    else:
        a = g.randint(-200, 30000 if dt.itemsize == 2 else 3000000, shape).astype(dt)
    if D > 1:
        a[:, :, 0] = 0
    if shape == (1, 1, 1):
        a[...] = 7
    return a


def rule(a, crop, slope, inter, inner):
    """the reference's statements in float64 -> stats (n, sum, ssd, vmax, nan_inner) and the three volumes (H', W', D)"""
    (h0, h1), (w0, w1) = crop
    H, W, D = a.shape
    img = a.astype(np.float64) * slope + inter
    vmax = np.nanmax(img)
    nan_inner = int(np.isnan(img[:, :, inner[0]:D - inner[1]]).sum())
    img = np.where(np.isnan(img), 0.0, img)
    img = img[h0:H - h1, w0:W - w1]
    mask = img > 0
    n = int(mask.sum())
    s = img.sum()
    norm = s / (n + 1)
    ssd = (mask * (img - norm) ** 2).sum()
    std = np.sqrt(ssd / (n + 1))
    z = (img - norm) / (std + 1e-8)
    z[~mask] = -10
    return (n, s, ssd, vmax, nan_inner), {'zscore': z, 'mean': img / norm, 'label': img}, mask


def as_input(a, order):
    """device tensor of the volume in the file's order (D, W, H) or in C order (H, W, D), in its own dtype"""
    arr = np.ascontiguousarray(a.transpose(2, 1, 0)) if order == 'file' else np.ascontiguousarray(a)
    return torch.from_numpy(arr).to(DEV)


def ulp_ok(got, want64):
    want = want64.astype(np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)


def check_stats(got, want, exact_sum, what):
    n, s, ssd, vmax, nan_inner = want
    assert got[0] == n and got[4] == nan_inner and got[3] == vmax, (what, got, want)
    if exact_sum:
        assert got[1] == s, (what, got[1], s)
    else:
        assert abs(got[1] - s) <= 1e-12 * abs(s), (what, got[1], s)
    assert abs(got[2] - ssd) <= 1e-12 * abs(ssd), (what, got[2], ssd)


def check_volume(got, want64, kind, mask, what):
    if kind == 'label':
        assert np.array_equal(got.view(np.int32), want64.astype(np.float32).view(np.int32)), what
        return
    ok = ulp_ok(got, want64)
    assert ok.all(), (what, int((~ok).sum()), float(np.abs(got - want64).max()))
    if kind == 'zscore':
        assert (got[~mask].view(np.int32) == np.float32(-10).view(np.int32)).all(), what


@pytest.mark.parametrize('kind', DTYPES)
@pytest.mark.parametrize('case', range(len(CASES)))
def test_stats_and_volumes_match_float64(mrdis, case, kind):
    shape, crop, inner = CASES[case]
    slope, inter = SCALES[kind]
    a = make_volume(shape, kind, seed=17 * case + len(kind) + ord(kind[0]))
    want_stats, want_vols, mask = rule(a, crop, slope, inter, inner)
    exact = np.dtype(kind).kind != 'f' and (slope, inter) == (1.0, 0.0)
    for order in ('file', 'c'):
        raw = as_input(a, order)
        c0 = mrdis.hip.launch_counts()
        stats = mrdis.prep_stats(raw, crop, slope, inter, order, inner)
        c1 = mrdis.hip.launch_counts()
        assert c1['prepstats'] == c0['prepstats'] + 1 and c1['prepwrite'] == c0['prepwrite']
        assert stats.dtype == torch.float64 and tuple(stats.shape) == (5,) and stats.device == raw.device
        check_stats(stats.cpu().numpy(), want_stats, exact, (shape, kind, order))
        assert torch.equal(stats, mrdis.prep_stats(raw, crop, slope, inter, order, inner))           # fixed order: the same bits
        for layout in ('dhw', 'hwd'):
            for k in KINDS:
                c1 = mrdis.hip.launch_counts()
                out = mrdis.prep_write(raw, stats, k, crop, layout, slope, inter, order)
                c2 = mrdis.hip.launch_counts()
                assert c2['prepwrite'] == c1['prepwrite'] + 1 and c2['prepstats'] == c1['prepstats']
                assert out.dtype == torch.float32 and out.is_contiguous()
                got = out.cpu().numpy()
                got = got.transpose(1, 2, 0) if layout == 'dhw' else got
                assert got.shape == want_vols[k].shape
                check_volume(np.ascontiguousarray(got), want_vols[k], k, mask, (shape, kind, order, layout, k))


def test_unaligned_and_strided_file_order_views(mrdis):
    """a file-order array that starts 2 bytes into an allocation (no 16-byte loads) and one cut out of a larger array (strides of the parent)"""
    shape, crop, inner = CASES[0]
    a = make_volume(shape, 'i2', seed=5)
    want_stats, want_vols, mask = rule(a, crop, 1.0, 0.0, inner)
    H, W, D = shape
    flat = torch.zeros(H * W * D + 1, dtype=torch.int16, device=DEV)
    flat[1:] = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 1, 0)).reshape(-1)).to(DEV)
    big = torch.zeros((D + 2, W + 3, H + 5), dtype=torch.int16, device=DEV)
    big[1:D + 1, 2:W + 2, 4:H + 4] = flat[1:].view(D, W, H)
    for raw in (flat[1:].view(D, W, H), big[1:D + 1, 2:W + 2, 4:H + 4]):
        stats = mrdis.prep_stats(raw, crop, inner=inner)
        check_stats(stats.cpu().numpy(), want_stats, True, tuple(raw.stride()))
        got = mrdis.prep_write(raw, stats, 'zscore', crop, 'hwd').cpu().numpy()
        check_volume(got, want_vols['zscore'], 'zscore', mask, tuple(raw.stride()))


def test_out_is_written_in_place_and_numpy_input_is_uploaded(mrdis):
    shape, crop, inner = CASES[0]
    a = make_volume(shape, 'f4', seed=8)
    _, want_vols, mask = rule(a, crop, 1.0, 0.0, inner)
    raw = np.ascontiguousarray(a.transpose(2, 1, 0))
    stats = mrdis.prep_stats(raw, crop, inner=inner, device=DEV)
    H2, W2, D = want_vols['zscore'].shape
    out = torch.full((D, H2, W2), 99.0, device=DEV)
    ptr = out.data_ptr()
    back = mrdis.prep_write(raw, stats, 'zscore', crop, 'dhw', out=out)
    assert back is out and out.data_ptr() == ptr
    check_volume(np.ascontiguousarray(out.cpu().numpy().transpose(1, 2, 0)), want_vols['zscore'], 'zscore', mask, 'out=')
    vol, stats2 = mrdis.prep_volume(raw, 'zscore', crop, 'dhw', inner=inner, device=DEV)
    assert torch.equal(vol, out) and torch.equal(stats2, stats)
    with pytest.raises(mrdis.MrdisError, match='out must be'):
        mrdis.prep_write(raw, stats, 'zscore', crop, 'hwd', out=out)


def test_prep_volume_reads_nothing_back(mrdis):
    shape, crop, inner = CASES[3]
    raw = as_input(make_volume(shape, 'i2', seed=2), 'file')
    mrdis.prep_volume(raw, 'zscore', crop, 'hwd', inner=inner)              # the workspace is allocated
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        vol, stats = mrdis.prep_volume(raw, 'zscore', crop, 'hwd', inner=inner)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert tuple(vol.shape) == (64, 64, 20) and bool(torch.isfinite(vol).all())


def test_unsupported_geometry_raises_before_any_launch(mrdis):
    before = mrdis.hip.launch_counts()
    stats = torch.zeros(5, dtype=torch.float64, device=DEV)
    tall = torch.zeros((2, 2, 1025), dtype=torch.int16, device=DEV)
    small = torch.zeros((4, 6, 8), dtype=torch.int16, device=DEV)
    for raw, crop in ((tall, ((0, 0), (0, 0))), (small, ((4, 4), (0, 0))), (small, ((0, 0), (1, 5))), (small, ((9, 0), (0, 0)))):
        with pytest.raises(mrdis.MrdisError, match='unsupported geometry'):
            mrdis.prep_stats(raw, crop)
        with pytest.raises(mrdis.MrdisError, match='unsupported geometry'):
            mrdis.prep_write(raw, stats, 'zscore', crop, 'dhw')
    with pytest.raises(mrdis.MrdisError):
        mrdis.prep_stats(small.to(torch.int64), ((0, 0), (0, 0)))
    with pytest.raises(mrdis.MrdisError):
        mrdis.prep_write(small, stats, 'median', ((0, 0), (0, 0)), 'dhw')
    assert mrdis.hip.launch_counts() == before


# ---------------------------------------------------------------------------------------------- trees of NIfTI files
def nifti_bytes(a, code, slope=1.0, inter=0.0):
    H, W, D = a.shape
    hdr = bytearray(352)
    struct.pack_into('<i', hdr, 0, 348)
    struct.pack_into('<8h', hdr, 40, 3, H, W, D, 1, 1, 1, 1)
    struct.pack_into('<2h', hdr, 70, code, 8 * a.dtype.itemsize)
    struct.pack_into('<8f', hdr, 76, 1, 1, 1, 1, 0, 0, 0, 0)
    struct.pack_into('<3f', hdr, 108, 352.0, slope, inter)
    hdr[344:348] = b'n+1\0'
    return bytes(hdr) + np.ascontiguousarray(a.transpose(2, 1, 0)).tobytes()


def scan(shape, g):
    """an MR-like int16 volume: positive inside an ellipse, 0 outside"""
    H, W, D = shape
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    inside = (((yy - H / 2 + 0.5) / (0.42 * H)) ** 2 + ((xx - W / 2 + 0.5) / (0.40 * W)) ** 2) <= 1
    return (g.randint(1, 3000, shape) * inside[:, :, None]).astype(np.int16)


def write_tree(root, n_good, shape, contrasts, bad=False, seed=1):
    """-> ({key: (H, W, D) raw array} of the good subjects, their ids); with `bad`, one subject with an all-zero contrast and one of another shape"""
    import gzip
    g = np.random.RandomState(seed)
    suffix = {'T1': 't1', 'T1c': 't1ce', 'T2': 't2', 'T2_FLAIR': 'flair', 'seg': 'seg'}
    arrays, good = {}, []
    names = [f'BraTS20_Training_{i:03d}' for i in range(n_good + (2 if bad else 0))]
    for i, subj in enumerate(names):
        os.makedirs(os.path.join(root, subj))
        is_zero, is_odd = bad and i == 3, bad and i == 7
        for c in list(contrasts) + ['seg']:
            if c == 'seg':
                a = (g.randint(0, 5, shape) * (g.rand(*shape) < 0.2)).astype(np.uint8)
                a[0, 0, 0] = 4
            else:
                a = scan((shape[0], shape[1] + 2, shape[2]) if is_odd and c == contrasts[-1] else shape, g)
                if is_zero and c == contrasts[0]:
                    a[...] = 0
            blob = nifti_bytes(a, 2 if c == 'seg' else 4)
            if i % 4 == 0:
                with gzip.open(os.path.join(root, subj, f'{subj}_{suffix[c]}.nii.gz'), 'wb', compresslevel=1) as f:
                    f.write(blob)
            else:
                with open(os.path.join(root, subj, f'{subj}_{suffix[c]}.nii'), 'wb') as f:
                    f.write(blob)
            if not (is_zero or is_odd):
                arrays[f'{subj}/{c}'] = a
        if not (is_zero or is_odd):
            good.append(subj)
    return arrays, good


@pytest.fixture(scope='module')
def tree13(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('raw13'))
    arrays, good = write_tree(root, 11, (64, 64, 16), ['T1', 'T2'], bad=True)
    return root, arrays, good


NO_CROP = ((0, 0), (0, 0))


@pytest.mark.parametrize('norm_type', ['z-score', 'mean'])
def test_build_store_from_raw(mrdis, tree13, norm_type):
    root, arrays, good = tree13
    lines = []
    store, kept = mrdis.build_store_from_raw(root, DEV, norm_type=norm_type, crop=NO_CROP, log=lines.append)
    assert kept == good and len(kept) == 11
    assert len(lines) == 2 and 'BraTS20_Training_003' in lines[0] and 'max 0' in lines[0] and 'BraTS20_Training_007' in lines[1] and 'shape' in lines[1]
    assert sorted(store.vols) == sorted(arrays) and store.shape == (64, 64, 16)
    want = {}
    for key, a in arrays.items():
        _, vols, mask = rule(a, NO_CROP, 1.0, 0.0, (50, 50))
        kind = 'label' if key.endswith('/seg') else ('mean' if norm_type == 'mean' else 'zscore')
        want[key] = (vols[kind], kind, mask)
    ref = mrdis.VolumeStore.from_arrays({k: v[0].astype(np.float32) for k, v in want.items()}, DEV)
    for key, (v, kind, mask) in want.items():
        got = store.vols[key]
        assert got.shape == ref.vols[key].shape == (16, 64, 64) and store.ptr(key) != 0
        check_volume(np.ascontiguousarray(got.cpu().numpy().transpose(1, 2, 0)), v, kind, mask, key)
    with pytest.raises(ValueError, match='shape'):
        store.add_device('x/T1', torch.zeros((16, 64, 65), device=DEV))
    with pytest.raises(ValueError):
        store.add_device('x/T1', torch.zeros((16, 64, 64), dtype=torch.float64, device=DEV))


def test_build_store3d_from_raw(mrdis, tree13):
    root, arrays, good = tree13
    store, kept = mrdis.build_store_from_raw(root, DEV, store_cls=mrdis.VolumeStore3D, crop=NO_CROP, contrasts=['T2'], subjects=good[:3],
                                             log=lambda *a: None)
    assert kept == good[:3] and sorted(store.vols) == sorted(f'{s}/{c}' for s in good[:3] for c in ('T2', 'seg')) and store.shape == (64, 64, 16)
    for key, got in store.vols.items():
        _, vols, mask = rule(arrays[key], NO_CROP, 1.0, 0.0, (50, 50))
        kind = 'label' if key.endswith('/seg') else 'zscore'
        assert tuple(got.shape) == (64, 64, 16)                        # (H, W, D): the layout VolumeStore3D keeps
        check_volume(got.cpu().numpy(), vols[kind], kind, mask, key)
    key = good[0] + '/T2'
    p = store.crop_min_ptr(key, 2, 9)
    mins, rows = store._mins[(2, 9)]
    assert p == mins.data_ptr() + 4 * rows[key] and float(mins[rows[key]]) == float(store.vols[key][:, :, 2:11].min()) == -10.0
    store.add_device('x/T2', store.vols[key].clone())
    assert not store._mins and store.crop_min_ptr('x/T2', 2, 9) != 0 and store.crop_min_ptr('y/T2', 2, 9) == 0


def test_run_trains_from_raw_files(mrdis, tmp_path):
    root = str(tmp_path / 'raw')
    os.makedirs(root)
    write_tree(root, 13, (64, 64, 16), ['T1', 'T2'], seed=4)
    data_path = tmp_path / 'lists'
    base = dict(contrast_list=['T1', 'T2'], input_height=64, input_width=64, batch_size=8, epochs=1, gpu='0', data_source='raw', raw_path=root,
                raw_slices=[3, 12], raw_crop=[[0, 0], [0, 0]], data_path=str(data_path), ckpt_root=str(tmp_path / 'ckpt'), ckpt_timelabel='t0')
    (tmp_path / 'train.yaml').write_text(yaml.dump(base))
    cfg = mrdis.train.setup_config(str(tmp_path / 'train.yaml'), device=DEV)
    run = mrdis.train.Run(cfg, log=lambda *a: None)
    for s in ('train', 'val', 'test'):
        assert (data_path / f'fold_BraTS_0_{s}_noval.txt').exists() and (data_path / f'fold_BraTS_3d_0_{s}_noval.txt').exists()
    subj, idx = mrdis.load_idx_list(str(data_path / 'fold_BraTS_0_train_noval.txt'))
    assert len(subj) == 10 * 9 and set(idx) == set(range(3, 12)) and len(run.loaders['train'].dataset) == 90
    run.train()
    stat = run.evaluate(phase='test', set_='test')
    assert np.isfinite(stat['recon_x_mix']) and np.isfinite(stat['all'])
    assert os.path.exists(os.path.join(cfg['ckpt_path'], 'epoch000.pth.tar'))


def test_run3d_steps_from_raw_files(mrdis, tmp_path):
    root = str(tmp_path / 'raw')
    os.makedirs(root)
    write_tree(root, 24, (32, 32, 123), ['T1', 'T2'], seed=6)
    data_path = tmp_path / 'lists'
    cfg = dict(dataset_name='BraTS', data_path=str(data_path), data_source='raw', raw_path=root, raw_crop=[[0, 0], [0, 0]], contrast_list=['T1', 'T2'],
               batch_size=2, model_name='NVNet3D', init_channels=8, epochs=1, max_batches=1, ckpt_path=str(tmp_path / 'ckpt'), device='cuda:0')
    run = mrdis.Run3D(cfg, log=lambda *a: None)
    assert isinstance(run.data.store, mrdis.VolumeStore3D) and run.data.store.shape == (32, 32, 123) and run.input_shape == (32, 32, 32)
    assert len(run.data.store.vols) == 24 * 3
    for s in ('train', 'val', 'test'):
        assert (data_path / f'fold_BraTS_3d_0_{s}_noval.txt').exists()
    run.train()
    assert np.isfinite(run.last_stat['loss']) and 0.0 <= run.last_stat['dice'] <= 1.0
