"""Rotated and zoomed training patches on the GPU (csrc/mrdis_warp.hip, patch3d.patch_warp, data3d.py's `patch_warp` keys, Run3D) against the
plain-numpy oracle tests/warp_check.py.  Exact: the targets, the positions of the -10 background marker, every row without a warp or with the
identity matrix (patch_gather's bits), quarter turns (torch.rot90 of the gathered patch), tiled against generic kernel, run against run.
Bounded: the interpolated intensities, per element within 18 * 2^-24 * (amax |scale| + |shift|) of the float64 oracle (derived at
warp_check.bound).  The kernel's worst ratio to that unit and the fp32 numpy oracle's, per case: profiles/warp_path_margins.txt, recorded
with MRDIS_DUMP_MEASURED=<dir> (tests do not write into the tree)."""
import numpy as np
import pytest
import torch

import patch3d_check as chk
import warp_check as wchk
from fixtures import dump_measured
from fixtures_data3d import data3d_volumes, data3d_subjects
from test_gpu_patch3d import Rows, dev, _volumes

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
CLASSES = (1, 2, 4)
NOFLIP = (False, False, False)


class WRows(Rows):
    """Rows with the five matrix words: `warp` = a (3, 3) int32 matrix sets the WARP flag, `matrix` alone stores words the kernel must ignore"""

    def add(self, vols, seg=None, warp=None, matrix=None, **kw):
        super().add(vols, seg, **kw)
        M, p = self.M, self.p
        a = warp if warp is not None else matrix
        row = np.concatenate([self.rows[-1], wchk.pack(a) if a is not None else np.zeros(p.WARP_EXTRA, np.int64)])
        if warp is not None:
            row[2 * M + 1] |= p.WARP
        self.rows[-1] = row


# ---------------------------------------------------------------- hand-built tables against the oracle
# name -> (M, volume, patch, tiled)
CASES = {
    'm4 cube': (4, (24, 20, 28), (16, 16, 16), True),             # the unrolled tile kernel; 4 x 4 x 1 bricks of 8 x 8 x 16, partial in h and w
    'm4 slab': (4, (24, 20, 28), (8, 16, 24), True),              # PD = 24: a partial brick along d
    'm2 cube': (2, (24, 20, 28), (16, 16, 16), True),             # the run-time tile kernel, bricks of 4 x 4 x 64 under four channels
    'm2 slab': (2, (24, 20, 28), (8, 16, 24), True),
    'generic': (3, (9, 11, 13), (5, 7, 9), False),                # 315 * 3 floats: no multiple of 4 -> one thread per float
    'whole': (4, (8, 16, 24), (8, 16, 24), True),                 # patch = volume: every rotated sample leaves it, clamping on all six faces
}
_REF = {}


def _case(name):
    """the items of a case and their oracle results, built once: six rows -- random warps at two opposite corners, the middle and a mixed corner
    (with flips, an absent contrast, a row without label volume, a row that is not augmented), the identity matrix, and a row without the flag"""
    if name in _REF:
        return _REF[name]
    M, shape, patch, _ = CASES[name]
    seed = sorted(CASES).index(name)
    rs = np.random.RandomState(100 + seed)
    vols, seg = _volumes(M, shape, 40 + seed)
    for v in vols:                                                  # (a scale per case: amax is part of the bound; -10 stays the minimum)
        tissue = v != -10.0
        v[tissue] = np.clip(v[tissue] * np.float32(1 + seed), -9.5, None)
        assert v.min() == -10.0
    top = tuple(n - p for n, p in zip(shape, patch))
    mid = tuple(t // 2 for t in top)
    rnd = lambda: wchk.matrix(rs.uniform(-30, 30, 3), rs.uniform(0.7, 1.4))
    items = [dict(vols=vols, seg=seg, origin=(0, 0, 0), warp=rnd(), flips=NOFLIP, aug=True, scale=1.07, shift=-0.04),
             dict(vols=[v if m != 1 else None for m, v in enumerate(vols)], seg=seg, origin=top, warp=rnd(), flips=(True, False, True), aug=True, scale=0.93, shift=0.08),
             dict(vols=vols, seg=None, origin=mid, warp=rnd(), flips=(False, True, False), aug=True, scale=1.0, shift=0.0),
             dict(vols=vols, seg=seg, origin=(0, top[1], 0), warp=wchk.matrix((30, -30, 30), 0.7), flips=(True, True, True), aug=False),
             dict(vols=vols, seg=seg, origin=mid, warp=wchk.IDENTITY, flips=(True, True, False), aug=True, scale=1.1, shift=0.05),
             dict(vols=vols, seg=seg, origin=top, warp=None, matrix=rnd(), flips=(False, False, True), aug=True, scale=0.9, shift=-0.1)]
    for it in items:
        a = it['warp'] if it['warp'] is not None else wchk.IDENTITY
        args = (a, it['origin'], patch, it['flips'])
        aug = (it['aug'], it.get('scale', 1.0), it.get('shift', 0.0))
        it['x64'], it['mask'], it['marker'] = wchk.warp_inputs(it['vols'], *args, *aug, np.float64)
        it['x32'] = wchk.warp_inputs(it['vols'], *args, *aug, np.float32)[0]
        it['t'] = {K: wchk.warp_targets(it['seg'], *args, K) for K in (0, 3)}
        it['unit'] = wchk.bound(it['vols'], aug[1], aug[2], units=1)
    _REF[name] = items
    return items


def _table(mrdis, name):
    M, shape, patch, _ = CASES[name]
    items = _case(name)
    rows = WRows(mrdis, M)
    for it in items:
        rows.add(it['vols'], it['seg'], warp=it['warp'], matrix=it.get('matrix'), flips=it['flips'], aug=it['aug'], scale=it.get('scale', 1.0), shift=it.get('shift', 0.0))
    origins = dev(np.array([tuple(it['origin']) + (-1,) for it in items]), np.int32)
    return rows, rows.table(), origins


def _run(mrdis, tab, origins, M, shape, patch):
    """inputs, mask, label targets, three region channels; one launch each, counted"""
    hip, p = mrdis.hip, mrdis.patch3d
    out = []
    for kw in ({}, dict(targets=True, relabel=True), dict(targets=True, K=3, relabel=True)):
        hip.launch_counts(reset=True)
        r = p.patch_warp(tab, origins, M, shape, patch, **kw)
        c = hip.launch_counts()
        assert c['patchwarp'] == 1 and c['all'] == 1 and c['patchgather'] == 0, c
        out.append(r)
    (x, mask), t, k = out
    return x, mask, t, k


@pytest.mark.parametrize('name', sorted(CASES))
def test_warp_against_the_oracle(mrdis, name):
    hip, p = mrdis.hip, mrdis.patch3d
    M, shape, patch, tiled = CASES[name]
    items = _case(name)
    rows, tab, origins = _table(mrdis, name)
    assert tab.shape[1] == 2 * M + 12
    x, mask, t, k = _run(mrdis, tab, origins, M, shape, patch)
    assert x.shape == (len(items), M) + patch and x.permute(0, 2, 3, 4, 1).is_contiguous() and k.permute(0, 2, 3, 4, 1).is_contiguous()
    # two runs give the same bits; the generic kernel gives the tiled kernel's
    x2, mask2, t2, k2 = _run(mrdis, tab, origins, M, shape, patch)
    assert torch.equal(x, x2) and torch.equal(mask, mask2) and torch.equal(t, t2) and torch.equal(k, k2)
    if tiled:
        hip.set_option('debug_volgen', 1)
        xg, maskg, tg, kg = _run(mrdis, tab, origins, M, shape, patch)
        hip.set_option('debug_volgen', 0)
        assert torch.equal(x.view(torch.int32), xg.view(torch.int32)) and torch.equal(mask, maskg) and torch.equal(t, tg) and torch.equal(k, kg)
    # rows with the flag clear and rows with the identity matrix: patch_gather's bits (it reads the first 2 M + 7 words of the same rows)
    gx, gmask = p.patch_gather(tab, origins, M, shape, patch)
    gt = p.patch_gather(tab, origins, M, shape, patch, targets=True, relabel=True)
    gk = p.patch_gather(tab, origins, M, shape, patch, targets=True, K=3, relabel=True)
    assert torch.equal(mask, gmask)
    same = [i for i, it in enumerate(items) if it['warp'] is None or it['warp'] is wchk.IDENTITY]
    assert len(same) == 2
    for i in same:
        assert torch.equal(x[i], gx[i]) and torch.equal(t[i], gt[i]) and torch.equal(k[i], gk[i]), i
    assert not torch.equal(x[0], gx[0]) and not torch.equal(t[0], gt[0])
    xn, tn, kn = x.cpu().numpy(), t.cpu().numpy(), k.cpu().numpy()
    np.testing.assert_array_equal(mask.cpu().numpy(), np.stack([it['mask'] for it in items]))
    failures = []
    for i, it in enumerate(items):
        np.testing.assert_array_equal(tn[i], it['t'][0], err_msg=f'{name} row {i}: label targets')
        np.testing.assert_array_equal(kn[i], it['t'][3], err_msg=f'{name} row {i}: region channels')
        marker = it['marker']
        np.testing.assert_array_equal(xn[i] == -10, marker | (it['x32'] == -10), err_msg=f'{name} row {i}: the -10 positions')
        assert (xn[i][marker] == -10).all()
        if it['aug'] and it['warp'] is not None:
            assert marker.any() and not marker.all(), (name, i)    # the background region touches the patch
        err = np.abs(xn[i].astype(np.float64) - it['x64'])
        ratio = float((err / it['unit']).max()) if it['unit'] > 0 else float(err.max())
        yard = float((np.abs(it['x32'].astype(np.float64) - it['x64']) / it['unit']).max()) if it['unit'] > 0 else 0.0
        bits = int((xn[i].view(np.uint32) != it['x32'].view(np.uint32)).sum())
        print(f'{name} row {i}: kernel {ratio:.3f} units, fp32 numpy {yard:.3f} units, {bits} of {xn[i].size} floats differ from fp32 numpy')
        dump_measured('warp_path_margins.jsonl', dict(case=name, row=i, M=M, shape=shape, patch=patch, warped=it['warp'] is not None and it['warp'] is not wchk.IDENTITY,
                                                      aug=it['aug'], kernel=ratio, fp32_numpy=yard, differ_from_fp32_numpy=bits, floats=int(xn[i].size)))
        if not (err <= 18 * it['unit']).all():
            failures.append(f'{name} row {i}: {ratio:.2f} units > 18 (fp32 numpy: {yard:.2f})')
    assert not failures, '\n'.join(failures)
    if name == 'whole':                                             # the rotated samples did leave the volume, through every face
        a = [[int(v) for v in r] for r in items[3]['warp']]
        for r in range(3):
            s = [((patch[r] - 1) << 16) + sum(a[r][c] * (2 * o[c] - (patch[c] - 1)) for c in range(3))
                 for o in [(i, j, k) for i in (0, patch[0] - 1) for j in (0, patch[1] - 1) for k in (0, patch[2] - 1)]]
            assert min(s) >> 17 < 0 and (max(s) >> 17) + 1 > shape[r] - 1, (r, s)


def test_quarter_turns_of_a_cube_equal_rot90_of_the_gathered_patch(mrdis):
    p = mrdis.patch3d
    M, shape, patch = 4, (24, 20, 28), (16, 16, 16)
    vols, seg = _volumes(M, shape, 60)
    turns = [((0, 0, 90), 3, (2, 3)), ((0, 0, -90), 1, (2, 3)), ((90, 0, 0), 3, (3, 4)), ((0, 90, 0), 3, (4, 2)), ((0, 0, 180), 2, (2, 3)), ((180, 0, 0), 2, (3, 4))]
    rows = WRows(mrdis, M)
    for i, (ang, _, _) in enumerate(turns):
        rows.add(vols, seg, warp=p.warp_matrix(ang, 1.0), aug=i != 2, scale=1.05, shift=0.02)
    tab = rows.table()
    origins = dev(np.array([(i, 4 - i % 4, 2 * i, -1) for i in range(len(turns))]), np.int32)
    x, _ = p.patch_warp(tab, origins, M, shape, patch)
    k3 = p.patch_warp(tab, origins, M, shape, patch, targets=True, K=3, relabel=True)
    t = p.patch_warp(tab, origins, M, shape, patch, targets=True)
    gx, _ = p.patch_gather(tab, origins, M, shape, patch)
    gk = p.patch_gather(tab, origins, M, shape, patch, targets=True, K=3, relabel=True)
    gt = p.patch_gather(tab, origins, M, shape, patch, targets=True)
    for i, (ang, k, dims) in enumerate(turns):
        assert torch.equal(x[i:i + 1], torch.rot90(gx[i:i + 1], k, dims)), ang
        assert torch.equal(k3[i:i + 1], torch.rot90(gk[i:i + 1], k, dims)), ang
        assert torch.equal(t[i:i + 1], torch.rot90(gt[i:i + 1], k, tuple(d - 1 for d in dims))), ang
        assert not torch.equal(x[i], gx[i])


def test_no_table_sends_a_read_outside_the_volume(mrdis):
    """entries far beyond any zoom (+-2^31) and origins outside the volume: the kernel clamps entries, origins and indices, so every value it
    returns is a value of the volume (not augmented: interpolation between volume values stays inside their range)"""
    p = mrdis.patch3d
    M, shape, patch = 4, (8, 16, 24), (8, 16, 16)
    vols, seg = _volumes(M, shape, 61, positive=True)
    wild = np.array([[2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1], [-2 ** 31, -2 ** 31, -2 ** 31], [2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1]], dtype=np.int32)
    rows = WRows(mrdis, M)
    rows.add(vols, seg, warp=wild)
    rows.add(vols, seg, warp=wild.T.copy(), flips=(True, True, True))
    tab = rows.table()
    far = dev(np.array([[2 ** 31 - 1, -2 ** 31, 99, -1], [-7, 99, -2 ** 31, -1]]), np.int32)
    for gen in (0, 1):
        mrdis.hip.set_option('debug_volgen', gen)
        x, _ = p.patch_warp(tab, far, M, shape, patch)
        t = p.patch_warp(tab, far, M, shape, patch, targets=True)
        torch.cuda.synchronize()
        x, t = x.cpu().numpy(), t.cpu().numpy()
        for m in range(M):                                          # (a rounded interpolation may pass its larger operand by an ulp)
            assert vols[m].min() * (1 - 1e-6) <= x[:, m].min() and x[:, m].max() <= vols[m].max() * (1 + 1e-6)
        assert set(np.unique(t)) <= set(np.unique(seg))
    mrdis.hip.set_option('debug_volgen', 0)


# ---------------------------------------------------------------- the loader
CONTRASTS = ['T1', 'T1c', 'T2', 'T2_FLAIR']


@pytest.fixture(scope='module')
def loader_world():
    data = data3d_volumes(n_subj=5, H=12, W=16, D=24, contrasts=CONTRASTS, seed=13)
    for k in [k for k in data if k.endswith('/seg')]:
        seg = np.zeros_like(data[k])
        rs = np.random.RandomState(len(k) + int(k[-7:-4]))
        seg.reshape(-1)[rs.choice(seg.size, 200, replace=False)] = rs.choice([1, 2, 4], 200)
        data[k] = seg
    return data, data3d_subjects(data)


def _loader(mrdis, world, **kw):
    data, subj = world
    store = mrdis.VolumeStore3D.from_arrays(data, DEV)
    ds = mrdis.VolumeDataset3D('BraTS', store, subj, CONTRASTS, aug=kw.pop('aug', True), dropoff=True)
    return mrdis.VolumeLoader3D(ds, 2, shuffle=False, region_channels=3, **kw)


@pytest.mark.parametrize('share', [1.0, 0.5])
def test_seeded_loader_gives_the_oracles_batches(mrdis, loader_world, share):
    hip = mrdis.hip
    data, subj = loader_world
    patch = (8, 8, 16)
    kw = dict(patch_fg=0.5, patch_flips='hwd', patch_warp=share, patch_rot=(30, 20, 10), patch_zoom=(0.7, 1.4))
    la = _loader(mrdis, loader_world, patch_size=patch, **kw)
    off = _loader(mrdis, loader_world, patch_size=patch, patch_fg=0.5, patch_flips='hwd')
    warped = []
    for epoch in range(2):
        np.random.seed(31 + epoch)
        list(off)                                                   # (prefix tables and minima are made outside the counted region)
        np.random.seed(31 + epoch)
        hip.launch_counts(reset=True)
        base = list(off)
        c = hip.launch_counts()
        assert c['patchorigin'] == 3 and c['patchgather'] == 6 and c['patchwarp'] == 0 and c['all'] == 9, c
        np.random.seed(31 + epoch)
        list(la)
        np.random.seed(31 + epoch)
        hip.launch_counts(reset=True)
        got = list(la)
        c = hip.launch_counts()
        assert c['patchorigin'] == 3 and c['patchgather'] == 0 and c['patchwarp'] == 6 and c['all'] == 9, c
        twin = np.random.RandomState(31 + epoch)
        want = wchk.loader_batches(data, subj, CONTRASTS, 2, patch, twin, aug=True, dropoff=True, K=3, **kw)
        assert np.random.get_state()[2] == twin.get_state()[2] and (np.random.get_state()[1] == twin.get_state()[1]).all()     # the same draws, no more
        assert len(got) == len(want) == 3
        # the feature moves no origin: the oracle's rule is patch3d_check.origin's, and the epoch's first item -- drawn before any warp draw --
        # has the origin it has with the feature off
        assert torch.equal(got[0]['origins'][0], base[0]['origins'][0])
        for b, w in zip(got, want):
            assert b['inputs'].shape == (len(w['inputs']), 4) + patch and b['inputs'].permute(0, 2, 3, 4, 1).is_contiguous()
            np.testing.assert_array_equal(b['origins'].cpu().numpy(), w['origins'])
            np.testing.assert_array_equal(b['targets'].cpu().numpy(), w['targets'])
            np.testing.assert_array_equal(b['mask'].cpu().numpy(), w['mask'])
            np.testing.assert_array_equal(b['mask_host'], w['mask'])
            x = b['inputs'].cpu().numpy()
            np.testing.assert_array_equal(x == -10, w['marker'])
            for i, (is_warped, bnd) in enumerate(zip(w['warped'], w['bound'])):
                warped.append(is_warped)
                if is_warped:
                    assert (np.abs(x[i].astype(np.float64) - w['inputs'][i]) <= bnd).all(), float(np.abs(x[i] - w['inputs'][i]).max() / bnd * 18)
                else:
                    np.testing.assert_array_equal(x[i], w['inputs32'][i])
    assert len(warped) == 10 and (all(warped) if share == 1.0 else {True, False} == set(warped))


def test_evaluation_loaders_never_launch_the_warp(mrdis, loader_world):
    hip = mrdis.hip
    ev = _loader(mrdis, loader_world, aug=False, patch_size=(8, 8, 16), patch_centre=True, patch_warp=1.0)
    noaug = _loader(mrdis, loader_world, aug=False, patch_size=(8, 8, 16), patch_warp=1.0)
    for la in (ev, noaug):
        assert not la.dataset.warps()
        np.random.seed(5)
        hip.launch_counts(reset=True)
        got = list(la)
        c = hip.launch_counts()
        assert len(got) == 3 and c['patchwarp'] == 0 and c['patchgather'] == 6 and c['patchorigin'] == 3, c
    np.random.seed(5)
    want = chk.loader_batches(loader_world[0], loader_world[1], CONTRASTS, 2, (8, 8, 16), np.random.RandomState(5), dropoff=True, K=3, centre=True)
    for b, w in zip(list(ev), want):
        np.testing.assert_array_equal(b['inputs'].cpu().numpy(), w['inputs'])
        np.testing.assert_array_equal(b['targets'].cpu().numpy(), w['targets'])


def test_three_launches_replay_through_a_graph_with_the_next_table(mrdis, loader_world):
    data, subj = loader_world
    patch = (8, 8, 16)
    la = _loader(mrdis, loader_world, patch_size=patch, patch_fg=0.5, patch_flips='hwd', patch_warp=0.5)
    st = la.dataset.store
    p = mrdis.patch3d
    np.random.seed(41)
    plans = [pl for _ in range(2) for pl in la.batch_plan() if len(pl[2]) == 2]
    tabs = [torch.from_numpy(la.patch_table(m)[0]).to(DEV) for _, _, m in plans]           # (builds the prefix tables and minima)
    assert len(tabs) == 4 and tabs[0].shape == (2, 20) and not torch.equal(tabs[0], tabs[1])
    flags = torch.stack(tabs)[:, :, 9] & p.WARP
    assert 0 < int((flags != 0).sum()) < 8                          # warped and unwarped rows are both replayed
    eager = []
    for tab in tabs:
        o = p.patch_origins(tab, 4, st.shape, patch, CLASSES)
        x, mask = p.patch_warp(tab, o, 4, st.shape, patch)
        eager.append((o, x, mask, p.patch_warp(tab, o, 4, st.shape, patch, targets=True, K=3, relabel=True)))
    static = tabs[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        o = p.patch_origins(static, 4, st.shape, patch, CLASSES)                          # warm-up outside the capture
        p.patch_warp(static, o, 4, st.shape, patch)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o = p.patch_origins(static, 4, st.shape, patch, CLASSES)
        x, mask = p.patch_warp(static, o, 4, st.shape, patch)
        t = p.patch_warp(static, o, 4, st.shape, patch, targets=True, K=3, relabel=True)
    for tab, (eo, ex, em, et) in zip(tabs[1:] + tabs[:1], eager[1:] + eager[:1]):
        static.copy_(tab)
        g.replay()
        assert torch.equal(o, eo) and torch.equal(x.view(torch.int32), ex.view(torch.int32)) and torch.equal(mask, em) and torch.equal(t, et)


# ---------------------------------------------------------------- Run3D
@pytest.fixture(scope='module')
def run_world(tmp_path_factory):
    data = data3d_volumes(n_subj=11, H=32, W=48, D=40, contrasts=CONTRASTS, seed=17)
    subj = data3d_subjects(data)
    root = tmp_path_factory.mktemp('warp3d')
    for name, part in (('train', subj[:5]), ('val', subj[5:8]), ('test', subj[8:11])):
        (root / f'fold_BraTS_3d_0_{name}_noval.txt').write_text('\n'.join(part) + '\n')
    return data, str(root), subj


def _run3d(mrdis, world, ckpt, **over):
    cfg = dict(dataset_name='BraTS', data_path=world[1], contrast_list=CONTRASTS, batch_size=2, model_name='NVNet3D', init_channels=8, epochs=2, lr=1e-4,
               ckpt_path=str(ckpt), device='cuda:0', seed=10, patch_size=[16, 16, 16], patch_fg=0.5, patch_flips='hwd')
    cfg.update(over)
    return mrdis.Run3D(cfg, store=mrdis.VolumeStore3D.from_arrays(world[0], DEV), log=lambda *a: None)


def test_run3d_trains_and_resumes_on_warped_patches(mrdis, run_world, tmp_path):
    hip = mrdis.hip
    straight = _run3d(mrdis, run_world, tmp_path / 'straight', patch_warp=0.5)
    tr, va = straight.loaders['train'].dataset, straight.loaders['val'].dataset
    assert tr.warps() and tr.patch_warp == 0.5 and not va.warps() and va.patch_warp == 0.0 and not straight.loaders['test'].dataset.warps()
    hip.launch_counts(reset=True)
    straight.train()
    c = hip.launch_counts()
    steps, vals = len(straight.loaders['train']), len(straight.loaders['val'])
    assert steps == 2 and vals == 1
    assert c['patchwarp'] == 4 * steps and c['patchgather'] == 4 * vals and c['patchorigin'] == 2 * (steps + vals) and c['volgather'] == 0, c
    assert 0 < straight.last_stat['dice'] < 1 and np.isfinite(straight.last_stat['loss'])
    first = _run3d(mrdis, run_world, tmp_path / 'resumed', patch_warp=0.5)
    first._train(1)                                                            # an interrupted run
    del first
    second = _run3d(mrdis, run_world, tmp_path / 'resumed', patch_warp=0.5, continue_train=True)
    assert second.start_epoch == 0
    second.train()
    a, b = straight.model.state_dict(), second.model.state_dict()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert straight.last_stat == second.last_stat


def test_run3d_with_the_feature_off_is_the_default_run(mrdis, run_world, tmp_path):
    hip = mrdis.hip
    default = _run3d(mrdis, run_world, tmp_path / 'default', epochs=1)
    default.train()
    hip.launch_counts(reset=True)
    off = _run3d(mrdis, run_world, tmp_path / 'off', epochs=1, patch_warp=0.0, patch_rot=[45, 0, 10], patch_zoom=[0.5, 2])
    off.train()
    c = hip.launch_counts()
    assert c['patchwarp'] == 0 and c['patchgather'] > 0, c
    a, b = default.model.state_dict(), off.model.state_dict()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert default.last_stat == off.last_stat
    on = _run3d(mrdis, run_world, tmp_path / 'on', epochs=1, patch_warp=1.0)
    on.train()
    assert any(not torch.equal(a[k], v) for k, v in on.model.state_dict().items())            # (the feature does reach the training batches)
