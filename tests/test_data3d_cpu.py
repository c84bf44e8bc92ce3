"""Host half of the 3-D loader (data3d.py) against batches of the reference's own ZeroDoseDataset3D + DataLoader
(tests/golden/data3d_b2.npz, tools/gen_golden_data3d.py): batch order, ids, masks, the augmentation draws and the position of the global RNG
stream; the list-file and file-name conventions of ZeroDoseDataAll3D; the data-parallel split.  No GPU."""
import os

import numpy as np
import pytest
import torch

from fixtures_data3d import DATA3D_CFG, data3d_volumes, data3d_subjects, compose_item, aug_bound

C = DATA3D_CFG


def _loaders(mrdis, data, **kw):
    store = mrdis.VolumeStore3D.from_arrays(data, 'cpu')
    subj = data3d_subjects(data)
    mk = lambda aug: mrdis.VolumeLoader3D(mrdis.VolumeDataset3D('BraTS', store, subj, C['contrasts'], aug=aug, dropoff=True),
                                          C['batch_size'], shuffle=True, **kw)
    return mk(True), mk(False)


def test_plan_matches_reference_loader(golden_dir):
    """same seeds -> the reference's batch order, ids and masks in every epoch; the drawn flip / scale / shift reproduce the recorded inputs within the
    fp32 bound with the identical -10 set; the global stream stands where the reference left it after every epoch."""
    import mrdis
    gold = np.load(os.path.join(golden_dir, 'data3d_b2.npz'))
    data = data3d_volumes()
    la, ln = _loaders(mrdis, data)
    z0, Dz = la.dataset.crop()
    assert (z0, Dz) == (45, C['D'] - 91)
    np.random.seed(C['np_seed']); torch.manual_seed(C['torch_seed'])
    worst, flips, present, sizes = 0.0, 0, set(), set()
    for kind, loader, epochs in (('a', la, C['aug_epochs']), ('n', ln, C['plain_epochs'])):
        for ep in range(epochs):
            n = 0
            for bi, (k, idxs, metas) in enumerate(loader.batch_plan()):
                tag = f'{kind}{ep}_{bi}'
                assert k == bi
                assert [m[0] for m in metas] == list(gold[f'subj_{tag}'])
                assert [m[1] for m in metas] == list(gold[f'slice_{tag}']) == [0] * len(metas)
                _, mask_host = loader.table(metas)
                np.testing.assert_array_equal(mask_host, gold[f'mask_{tag}'])
                present |= set(mask_host.sum(1).astype(int).tolist()); sizes.add(len(metas))
                for r, (sid, _, ptrs, drop, tptr, flip, scale, shift) in enumerate(metas):
                    assert (flip, scale, shift) == (False, 1.0, 0.0) or kind == 'a'
                    x, raw, tgt = compose_item(data, sid, C['contrasts'], drop, flip, scale, shift, kind == 'a', z0, Dz)
                    ref = gold[f'inputs_{tag}'][r]
                    np.testing.assert_array_equal(tgt, gold[f'targets_{tag}'][r])
                    np.testing.assert_array_equal(x == -10, ref == -10)
                    if kind == 'n':
                        np.testing.assert_array_equal(x, ref)
                    else:
                        flips += flip
                        err, bound = np.abs(x.astype(np.float64) - ref), aug_bound(raw, scale, shift)
                        live = ref != -10
                        assert (err[live] <= bound[live]).all()
                        worst = max(worst, float((err[live] / bound[live]).max()))
                n += 1
            assert n == int(gold[f'nbatch_{kind}{ep}'])
            assert np.random.rand() == float(gold[f'next_rand_{kind}{ep}'])
    print(f'worst error / bound {worst:.3f}; flipped items {flips}')
    assert present == {1, 2, 3} and sizes == {1, 2} and 0 < flips < 15        # what the fixture was built to cover


def test_subject_list_drops_its_first_line(tmp_path):
    """the reference reads the list with pandas' default header handling (util.py:842): the first subject is taken as a header"""
    import mrdis
    p = tmp_path / 'fold_BraTS_3d_0_train_noval.txt'
    p.write_text('BraTS20_Training_001\nBraTS20_Training_002\nBraTS20_Training_003\n')
    assert list(mrdis.load_subj_list(str(p))) == ['BraTS20_Training_002', 'BraTS20_Training_003']


def test_file_names_and_loader_flags(tmp_path):
    import mrdis
    V = mrdis.VolumeData3D
    assert V.file_names('BraTS', 'mean', 3) == ('BraTS_All.h5', 'fold_BraTS_3d_3_train_noval.txt', 'fold_BraTS_3d_3_val_noval.txt',
                                                 'fold_BraTS_3d_3_test_noval.txt')
    assert V.file_names('BraTS', 'zscore', 0)[0] == 'BraTS_All_zscore_10.h5'
    assert V.file_names('ZeroDose', 'mean', 1) == ('ZeroDose_FDG_All_1103_norm.h5',) + ('ZeroDose_3d_all.txt',) * 3
    assert V.file_names('ZeroDose', 'zscore', 1)[0] == 'ZeroDose_FDG_All_1103_zscore_10.h5'
    with pytest.raises(ValueError):
        V.file_names('Tau')
    with pytest.raises(ValueError):
        V('NCANDA', str(tmp_path), store=object())
    data = data3d_volumes()
    subj = data3d_subjects(data)
    for s, names in (('train', subj), ('val', subj[:3]), ('test', subj[:2])):
        (tmp_path / f'fold_BraTS_3d_2_{s}_noval.txt').write_text('\n'.join(names) + '\n')
    store = mrdis.VolumeStore3D.from_arrays(data, 'cpu')
    d = V('BraTS', str(tmp_path), norm_type='zscore', batch_size=2, fold=2, shuffle=True, contrast_list=C['contrasts'], aug=True, dropoff=True,
          store=store)
    flags = lambda l: (l.dataset.aug, l.dataset.dropoff, l.shuffle, len(l.dataset))
    assert flags(d.trainLoader) == (True, True, True, 4)             # one less than the file has: the header quirk
    assert flags(d.valLoader) == (False, True, False, 2)
    assert flags(d.testLoader) == (False, False, False, 1)
    assert d.trainLoader.dataset.subj_list == subj[1:]
    assert len(d.trainLoader) == 2                                   # the partial last batch is served
    with pytest.raises(RuntimeError, match='h5py'):
        V('BraTS', str(tmp_path), fold=2, device='cpu')
    zd = mrdis.VolumeDataset3D('ZeroDose', store, subj, C['contrasts'])
    assert zd.crop() == (45, C['D'] - 92)


def _plan(mrdis, data, epochs, **kw):
    np.random.seed(11); torch.manual_seed(13)
    la, _ = _loaders(mrdis, data, **kw)
    seen = {}
    for ep in range(epochs):
        for k, idxs, metas in la.batch_plan():
            seen[(ep, k)] = (idxs, [(m[0], m[3], m[5], m[6], m[7]) for m in metas], la.table(metas)[1].tolist())
    return seen, float(np.random.rand())


def test_world_two_ranks_share_draws_and_split_batches():
    """both ranks see the same ids, masks and augmentation draws for batch k, drawn from the loader's own stream, and together serve every batch once"""
    import mrdis
    data = data3d_volumes()
    (s0, g0), (s1, g1) = _plan(mrdis, data, 2, rank=0, world=2), _plan(mrdis, data, 2, rank=1, world=2)
    assert g0 == g1                                      # the global stream moved alike on both ranks (the one seed draw of the loader's stream)
    assert all(k % 2 == 0 for _, k in s0) and all(k % 2 == 1 for _, k in s1)
    assert sorted(set(s0) | set(s1)) == [(ep, k) for ep in range(2) for k in range(3)]
    # the draws of batch k do not depend on the rank that serves it: a three-rank world walks the same global sequence, split differently
    both = {**s0, **s1}
    for r in range(3):
        s3, g3 = _plan(mrdis, data, 2, rank=r, world=3)
        assert g3 == g0
        for key, val in s3.items():
            assert both[key] == val
    flips = [f for v in both.values() for _, _, f, _, _ in v[1]]
    assert any(flips) and not all(flips)
