"""Rotated and zoomed training patches, the part that needs no GPU: the matrix and its packing, the numpy oracle (tests/warp_check.py) against
the unwarped cut and exact quarter turns, the loader's draw order with the feature off and on, the table layout, the keys' refusals and the
binding's refusals on the stub-library pattern of test_hip_contracts_cpu.py."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
import mrdis                                                    # noqa: E402
import patch3d_check as chk                                     # noqa: E402
import warp_check as wchk                                       # noqa: E402
from test_hip_contracts_cpu import install_stub, meta, put, short, strided, tensors, to, z, COMPUTE      # noqa: E402

hip = mrdis.hip
patch3d = mrdis.patch3d
F32, I32, I64 = torch.float32, torch.int32, torch.int64
NOFLIP = (False, False, False)


# ---------------------------------------------------------------- the matrix
def test_warp_matrix_identity_quarter_turn_and_zoom():
    a = patch3d.warp_matrix((0, 0, 0), 1)
    assert a.dtype == np.int32 and a.shape == (3, 3) and a.tolist() == [[65536, 0, 0], [0, 65536, 0], [0, 0, 65536]]
    assert patch3d.warp_matrix((0, 0, 90), 1.0).tolist() == [[0, -65536, 0], [65536, 0, 0], [0, 0, 65536]]
    assert patch3d.warp_matrix((90, 0, 0), 1.0).tolist() == [[65536, 0, 0], [0, 0, -65536], [0, 65536, 0]]
    assert patch3d.warp_matrix((0, 90, 0), 1.0).tolist() == [[0, 0, 65536], [0, 65536, 0], [-65536, 0, 0]]
    assert patch3d.warp_matrix((0, 0, 0), 2.0).tolist() == [[32768, 0, 0], [0, 32768, 0], [0, 0, 32768]]       # zoom 2 samples half the region
    assert patch3d.warp_matrix((0, 0, 0), 0.5)[0, 0] == 131072
    # the order R_h R_w R_d: a quarter turn about W after one about D, by hand -- R_h = I, R_w R_d = [[0, 0, 1], [1, 0, 0], [0, 1, 0]]
    assert patch3d.warp_matrix((0, 90, 90), 1.0).tolist() == [[0, 0, 65536], [65536, 0, 0], [0, 65536, 0]]
    # 30 degrees about D at zoom 1: cos = 0.8660254 -> floor(56755.84 + 0.5) = 56756, sin = 0.5 -> 32768
    assert patch3d.warp_matrix((0, 0, 30), 1.0).tolist() == [[56756, -32768, 0], [32768, 56756, 0], [0, 0, 65536]]
    rs = np.random.RandomState(0)
    for _ in range(200):
        ang, zoom = rs.uniform(-45, 45, 3), rs.uniform(0.5, 2)
        assert (patch3d.warp_matrix(ang, zoom) == wchk.matrix(ang, zoom)).all()
    assert mrdis.warp_matrix is patch3d.warp_matrix and mrdis.patch_warp is patch3d.patch_warp
    for bad in (((1, 2), 1.0), ((1, 2, 3), 0.0), ((1, 2, 3), -1.0), ((1, 2, float('nan')), 1.0), ('abc', 1.0), ((1, 2, 3), 1e-9)):
        with pytest.raises(ValueError, match='warp_matrix'):
            patch3d.warp_matrix(*bad)


def test_packing_of_negative_entries():
    a = np.array([[1, -1, 2], [-2, 65536, -65536], [-2 ** 31, 2 ** 31 - 1, -3]], dtype=np.int32)
    w = patch3d.pack_warp(a)
    assert w.dtype == np.int64 and w.shape == (5,) == (patch3d.WARP_EXTRA,)
    u = [int(v) & 0xffffffffffffffff for v in w]
    assert u[0] == 1 | 0xffffffff << 32                               # -1 fills its own 32 bits and no bit of its neighbour
    assert u[1] == 2 | 0xfffffffe << 32
    assert u[2] == 65536 | 0xffff0000 << 32
    assert u[3] == 0x80000000 | 0x7fffffff << 32
    assert u[4] == 0xfffffffd                                         # the last high half is zero
    assert (w == wchk.pack(a)).all()
    back = [(u[e // 2] >> (32 * (e % 2))) & 0xffffffff for e in range(9)]
    assert [b - (1 << 32) if b >= 1 << 31 else b for b in back] == a.reshape(-1).tolist()
    for bad in (a.astype(np.int64), a[:2], a.reshape(-1)):
        with pytest.raises(ValueError, match='pack_warp'):
            patch3d.pack_warp(bad)


# ---------------------------------------------------------------- the oracle
def _volume(shape, seed):
    rs = np.random.RandomState(seed)
    v = rs.randn(*shape).astype(np.float32)
    v[rs.rand(*shape) < 0.3] = -10.0
    return v, rs.randint(0, 5, size=shape).astype(np.float32)


def test_oracle_coordinates_by_hand():
    """patch (1, 1, 4) at origin (0, 0, 3) of a (1, 1, 10) volume, zoom 2 along d only: s = ((2 * 3 + 3) << 16) + 32768 (2 k - 3), in 2^-17
    voxels: k = 0 .. 3 -> 3.75, 4.25, 4.75, 5.25"""
    a = np.array([[65536, 0, 0], [0, 65536, 0], [0, 0, 32768]], np.int32)
    lo, hi, near, frac = wchk.coords(a, (0, 0, 3), (1, 1, 4), (1, 1, 10))
    assert lo[2].reshape(-1).tolist() == [3, 4, 4, 5] and hi[2].reshape(-1).tolist() == [4, 5, 5, 6]
    assert near[2].reshape(-1).tolist() == [4, 4, 5, 5] and (frac[2].reshape(-1) / wchk.ONE).tolist() == [0.75, 0.25, 0.75, 0.25]
    assert not lo[:2].any() and not hi[:2].any() and not frac[:2].any()                 # extents of 1: clamped onto index 0
    # zoom 0.5 leaves the volume on both sides: -1.5 -> floor -2, clamped; a half rounds up: nearest(2.5) = 3
    a = np.array([[65536, 0, 0], [0, 65536, 0], [0, 0, 131072]], np.int32)
    lo, hi, near, frac = wchk.coords(a, (0, 0, 0), (1, 1, 4), (1, 1, 4))                # s / 2^17 = 1.5 + 2 (k - 1.5) = -1.5, 0.5, 2.5, 4.5
    assert lo[2].reshape(-1).tolist() == [0, 0, 2, 3] and hi[2].reshape(-1).tolist() == [0, 1, 3, 3] and near[2].reshape(-1).tolist() == [0, 1, 3, 3]
    assert (frac[2].reshape(-1) / wchk.ONE).tolist() == [0.5] * 4
    # the D flip mirrors o before the matrix
    _, _, nf, _ = wchk.coords(a, (0, 0, 0), (1, 1, 4), (1, 1, 4), (False, False, True))
    assert nf[2].reshape(-1).tolist() == [3, 3, 1, 0]
    v = np.array([[[0, 10, 20, 40]]], np.float32)
    x, mask, marker = wchk.warp_inputs([v], np.array([[65536, 0, 0], [0, 65536, 0], [0, 0, 32768]], np.int32), (0, 0, 0), (1, 1, 4), dtype=np.float32)
    assert x.reshape(-1).tolist() == [7.5, 12.5, 17.5, 25.0] and mask.tolist() == [1] and not marker.any()     # 0.75, 1.25, 1.75, 2.25
    # the marker rule: m0 = 0 is the nearest voxel of the first output only; the corner 0 of the second output takes the nearest value 10
    x, _, marker = wchk.warp_inputs([v], np.array([[65536, 0, 0], [0, 65536, 0], [0, 0, 32768]], np.int32), (0, 0, 0), (1, 1, 4), aug=True, scale=2.0, shift=1.0)
    assert marker.reshape(-1).tolist() == [False] * 4 and x.reshape(-1).tolist() == [21.0, 26.0, 36.0, 51.0]    # nearest(0.75) = 1: 10 replaces the 0
    x, _, marker = wchk.warp_inputs([v], np.array([[65536, 0, 0], [0, 65536, 0], [0, 0, 65536 + 32768]], np.int32), (0, 0, 0), (1, 1, 4), aug=True)
    assert marker.reshape(-1).tolist() == [True, False, False, False] and x.reshape(-1)[0] == -10               # -0.75 -> clamped nearest 0


def test_oracle_identity_is_the_cut_and_quarter_turns_are_rot90():
    shape, patch = (9, 11, 13), (5, 7, 9)
    vol, seg = _volume(shape, 1)
    for flips in (NOFLIP, (True, False, True), (False, True, False)):
        for o in ((0, 0, 0), (4, 4, 4), (1, 2, 3)):
            for dtype in (np.float32, np.float64):
                x, mask, marker = wchk.warp_inputs([vol, None], wchk.IDENTITY, o, patch, flips, True, 1.1, 0.05, dtype)
                want, wmask = chk.gather_inputs([vol, None], o, patch, flips, True, 1.1, 0.05)
                if dtype is np.float32:
                    assert x.dtype == np.float32 and np.array_equal(x.view(np.uint32), want.view(np.uint32))     # bit for bit
                assert np.array_equal(marker, want == -10) and np.array_equal(mask, wmask)
            raw = wchk.warp_inputs([vol], wchk.IDENTITY, o, patch, flips, dtype=np.float32)[0]
            assert np.array_equal(raw[0], chk.cut(vol, o, patch, flips))
            for K in (0, 3):
                assert np.array_equal(wchk.warp_targets(seg, wchk.IDENTITY, o, patch, flips, K), chk.gather_targets(seg, o, patch, flips, K))
    # +90 degrees about D with a cubic patch: every fraction is 0 and the result is np.rot90(cut, 3) in the (h, w) plane
    a90 = patch3d.warp_matrix((0, 0, 90), 1.0)
    cube, o = (5, 5, 5), (2, 3, 4)
    assert not wchk.coords(a90, o, cube, shape)[3].any()
    x = wchk.warp_inputs([vol], a90, o, cube, dtype=np.float32)[0][0]
    assert np.array_equal(x, np.rot90(chk.cut(vol, o, cube, NOFLIP), 3, axes=(0, 1)))
    assert np.array_equal(wchk.warp_targets(seg, a90, o, cube, relabel=False), np.rot90(chk.cut(seg, o, cube, NOFLIP), 3, axes=(0, 1)))
    for cube, o in (((6, 6, 6), (1, 2, 3)), ((4, 4, 4), (5, 7, 9))):                    # an even extent: the centre lies between voxels, still exact
        for ang, k, axes in (((0, 0, 90), 3, (0, 1)), ((0, 0, -90), 1, (0, 1)), ((90, 0, 0), 3, (1, 2)), ((0, 90, 0), 3, (2, 0)), ((0, 0, 180), 2, (0, 1))):
            a = patch3d.warp_matrix(ang, 1.0)
            assert not wchk.coords(a, o, cube, shape)[3].any()
            x = wchk.warp_inputs([vol], a, o, cube, dtype=np.float32)[0][0]
            assert np.array_equal(x, np.rot90(chk.cut(vol, o, cube, NOFLIP), k, axes=axes)), ang


def test_fp32_oracle_stays_inside_the_bound_of_the_float64_one():
    """the bound the GPU test holds the kernel to, held first against the same rule in fp32 numpy"""
    shape, patch = (12, 10, 14), (8, 8, 8)
    vol, _ = _volume(shape, 2)
    vols = [vol, _volume(shape, 3)[0] * 3]
    rs = np.random.RandomState(4)
    worst = 0.0
    for _ in range(10):
        a = wchk.matrix(rs.uniform(-30, 30, 3), rs.uniform(0.7, 1.4))
        o = tuple(int(v) for v in rs.randint(0, np.array(shape) - patch + 1))
        scale, shift = 1 + 0.2 * (rs.rand() - 0.5), 0.2 * (rs.rand() - 0.5)
        x64, _, m64 = wchk.warp_inputs(vols, a, o, patch, NOFLIP, True, scale, shift, np.float64)
        x32, _, m32 = wchk.warp_inputs(vols, a, o, patch, NOFLIP, True, scale, shift, np.float32)
        assert np.array_equal(m64, m32) and (x64[m64] == -10).all() and m64.any() and not m64.all()
        worst = max(worst, float(np.abs(x32.astype(np.float64) - x64).max() / wchk.bound(vols, scale, shift, units=1)))
    assert 0 < worst <= 18, worst


# ---------------------------------------------------------------- the loader's draws
class RecordingStream:
    """a np.random.RandomState that notes which method made each draw, and how many values"""

    def __init__(self, seed):
        self.rs, self.calls = np.random.RandomState(seed), []

    def rand(self, *n):
        self.calls.append(('rand',) + n)
        return self.rs.rand(*n)

    def choice(self, a, n):
        self.calls.append(('choice',))
        return self.rs.choice(a, n)

    def randint(self, lo, hi, size, dtype):
        self.calls.append(('randint', size))
        return self.rs.randint(lo, hi, size=size, dtype=dtype)


def small_store(n_subj=3, shape=(6, 8, 10)):
    rs = np.random.RandomState(1)
    data = {}
    for s in range(n_subj):
        for c in ('T1', 'T2'):
            data[f's{s}/{c}'] = rs.randn(*shape).astype(np.float32)
        data[f's{s}/seg'] = rs.randint(0, 5, size=shape).astype(np.float32)
    del data['s1/T2']
    return data, mrdis.VolumeStore3D.from_arrays(data, 'cpu')


def _same_state(a, b):
    return a.get_state()[2] == b.get_state()[2] and (a.get_state()[1] == b.get_state()[1]).all()


def test_draws_with_the_feature_off_are_todays():
    """patch_warp = 0 (the default, and spelled out): the metas and the stream are patch3d_check.draw_item's, which has no warp draw"""
    data, store = small_store()
    for kw in ({}, {'patch_warp': 0.0, 'patch_rot': (45, 0, 10), 'patch_zoom': (0.5, 2)}):
        ds = mrdis.VolumeDataset3D('BraTS', store, ['s0', 's1', 's2'], contrast_list=['T1', 'T2'], aug=True, dropoff=True, patch_size=(2, 4, 4),
                                   patch_fg=0.5, patch_flips='hwd', **kw)
        assert ds.patch_warp == 0.0 and not ds.warps()
        for seed in range(8):
            for idx in range(3):
                rec, twin = RecordingStream(seed), np.random.RandomState(seed)
                m = ds.meta(idx, rec)
                drop, fg, u, fl, scale, shift = chk.draw_item(twin, 1 if idx == 1 else 2, True, True, 0.5, 'hwd')
                assert len(m) == 9 and len(m[8]) == 4 and m[3] == drop and m[8][0] == fg and m[8][1].tolist() == u.tolist() and m[8][2] == fl
                assert (m[5], m[6], m[7]) == (fl[0], scale, shift) and _same_state(rec.rs, twin)
                assert ('rand', 5) not in rec.calls
    ds.set_patch((2, 4, 4), patch_flips='hwd')                       # (no foreground share: a prefix table would be a kernel launch)
    loader = mrdis.VolumeLoader3D(ds, 2)
    assert loader.patch_table([ds.meta(0), ds.meta(1)])[0].shape == (2, 2 * 2 + patch3d.TABLE_EXTRA)


def test_five_more_doubles_per_item_whatever_the_first_says():
    data, store = small_store()
    rot, zoom = (30.0, 20.0, 10.0), (0.7, 1.4)
    for share in (1.0, 0.5, 1e-9):                                   # 1e-9: a warp is (all but) never drawn; the five doubles always are
        for dropoff, fg, flips in ((True, 0.5, 'hwd'), (False, 0.0, '')):
            on = mrdis.VolumeDataset3D('BraTS', store, ['s0', 's1', 's2'], contrast_list=['T1', 'T2'], aug=True, dropoff=dropoff, patch_size=(2, 4, 4),
                                       patch_fg=fg, patch_flips=flips, patch_warp=share, patch_rot=rot, patch_zoom=zoom)
            assert on.warps()
            seen = set()
            for seed in range(16):
                for idx in range(3):
                    rec, twin = RecordingStream(seed), np.random.RandomState(seed)
                    m = on.meta(idx, rec)
                    drop, is_fg, u, fl, scale, shift, warp = wchk.draw_item(twin, 1 if idx == 1 else 2, dropoff, True, fg, flips, share, rot, zoom)
                    assert _same_state(rec.rs, twin)
                    assert rec.calls.count(('rand', 5)) == 1 and rec.calls[-3:] == [('rand', 5), ('rand',), ('rand',)]      # after the flips, before scale and shift
                    assert len(m[8]) == 7 and m[8][:4] == (is_fg, m[8][1], fl, False) and m[8][1].tolist() == u.tolist() and (m[3], m[6], m[7]) == (drop, scale, shift)
                    assert m[8][4] is warp[0] and m[8][5] == warp[1] and m[8][6] == warp[2]
                    assert all(abs(a) <= r for a, r in zip(m[8][5], rot)) and zoom[0] <= m[8][6] <= zoom[1]
                    seen.add(m[8][4])
                    # the same item without the feature: drop, fg, u and the flips are the same draws, and the stream ends exactly five
                    # doubles earlier (the generator's state is its position: today's draws plus five doubles reach the same state)
                    off_rs = np.random.RandomState(seed)
                    base = chk.draw_item(off_rs, 1 if idx == 1 else 2, dropoff, True, fg, flips)
                    assert base[:4] == (drop, is_fg, base[2], fl) and base[2].tolist() == u.tolist()
                    assert not _same_state(off_rs, twin)
                    off_rs.rand(4)
                    assert not _same_state(off_rs, twin)
                    off_rs.rand()
                    assert _same_state(off_rs, twin)
            assert seen == ({True} if share == 1.0 else {False} if share == 1e-9 else {True, False})
    # by hand: r = rand(5) -> warp, angles, zoom
    ds = mrdis.VolumeDataset3D('BraTS', store, ['s0'], contrast_list=['T1'], aug=True, patch_size=(2, 4, 4), patch_flips='', patch_warp=0.5, patch_rot=rot, patch_zoom=zoom)
    rs = np.random.RandomState(3)
    m = ds.meta(0, rs)
    twin = np.random.RandomState(3)
    twin.randint(0, 2 ** 32, size=5, dtype=np.uint32)
    r = twin.rand(5)
    assert m[8][4] == bool(r[0] < 0.5) and m[8][5] == tuple((2 * r[1 + a] - 1) * rot[a] for a in range(3)) and m[8][6] == 0.7 + r[4] * (1.4 - 0.7)


def test_no_aug_and_centre_loaders_draw_nothing_for_the_warp():
    data, store = small_store()
    kw = dict(contrast_list=['T1', 'T2'], patch_size=(2, 4, 4), patch_warp=1.0)
    centre = mrdis.VolumeDataset3D('BraTS', store, ['s0', 's1', 's2'], dropoff=True, aug=True, patch_centre=True, **kw)
    noaug = mrdis.VolumeDataset3D('BraTS', store, ['s0', 's1', 's2'], aug=False, **kw)
    assert not centre.warps() and not noaug.warps()
    rec = RecordingStream(3)
    metas = [centre.meta(i, rec) for i in range(3)]
    assert ('rand', 5) not in rec.calls and ('randint', 5) not in rec.calls and all(len(m[8]) == 4 and m[8][3] is True for m in metas)
    rec = RecordingStream(3)
    metas = [noaug.meta(i, rec) for i in range(3)]
    assert rec.calls == [('randint', 5)] * 3 and all(len(m[8]) == 4 for m in metas)
    assert mrdis.VolumeLoader3D(noaug, 2).patch_table(metas[:2])[0].shape == (2, 4 + patch3d.TABLE_EXTRA)


class _Lists:
    """the fold lists VolumeData3D reads, written into a temporary directory"""

    def __init__(self, tmp_path, subj):
        for name in ('train', 'val', 'test'):
            (tmp_path / f'fold_BraTS_3d_0_{name}_noval.txt').write_text('header\n' + '\n'.join(subj) + '\n')
        self.path = str(tmp_path)


def test_volume_data_passes_the_keys_to_the_train_loader_only(tmp_path):
    data, store = small_store()
    lists = _Lists(tmp_path, ['s0', 's1', 's2'])
    d = mrdis.VolumeData3D('BraTS', lists.path, norm_type='z-score', batch_size=2, contrast_list=['T1', 'T2'], aug=True, dropoff=True, store=store, device='cpu',
                           patch_size=(2, 4, 4), patch_fg=0.5, patch_warp=0.25, patch_rot=(10, 20, 30), patch_zoom=(0.9, 1.1))
    tr, va, te = d.trainLoader.dataset, d.valLoader.dataset, d.testLoader.dataset
    assert (tr.patch_warp, tr.patch_rot, tr.patch_zoom) == (0.25, (10.0, 20.0, 30.0), (0.9, 1.1)) and tr.warps()
    assert va.patch_warp == te.patch_warp == 0.0 and not va.warps() and not te.warps() and va.patch_centre and te.patch_centre
    off = mrdis.VolumeData3D('BraTS', lists.path, norm_type='z-score', batch_size=2, contrast_list=['T1', 'T2'], aug=True, store=store, device='cpu', patch_size=(2, 4, 4))
    assert off.trainLoader.dataset.patch_warp == 0.0 and not off.trainLoader.dataset.warps()


# ---------------------------------------------------------------- the table
def test_table_layout_on_and_off():
    data, store = small_store()
    M = 2
    mk = lambda **kw: mrdis.VolumeLoader3D(mrdis.VolumeDataset3D('BraTS', store, ['s0', 's1'], contrast_list=['T1', 'T2'], aug=True), 2, patch_size=(2, 4, 4),
                                           patch_flips='wd', **kw)
    u = np.array([1, 2, 3, 2 ** 32 - 1, 5], np.uint32)
    head = lambda sid, flips: (sid, 0, [store.ptr(sid + '/T1'), store.ptr(sid + '/T2')], -1, store.ptr(sid + '/seg'), False, 1.25, -0.5)
    ang, zoom = (-10.0, 20.0, -30.0), 0.7
    metas_on = [head('s0', None) + ((False, u, (False, True, True), False, True, ang, zoom),),
                head('s1', None) + ((False, u, (False, False, False), False, False, (5.0, 5.0, 5.0), 1.3),)]
    metas_off = [m[:8] + (m[8][:4],) for m in metas_on]
    on, off = mk(patch_warp=0.5), mk()
    t_on, mask_on = on.patch_table(metas_on)
    t_off, mask_off = off.patch_table(metas_off)
    assert t_off.shape == (2, 2 * M + patch3d.TABLE_EXTRA) and t_on.shape == (2, 2 * M + patch3d.TABLE_EXTRA + patch3d.WARP_EXTRA) == (2, 2 * M + 12)
    assert t_on.dtype == np.int64 and np.array_equal(mask_on, mask_off)
    # the first 2 M + 7 words are today's, but for the flag
    keep = [c for c in range(2 * M + 7) if c != 2 * M + 1]
    assert np.array_equal(t_on[:, keep], t_off[:, keep])
    assert t_off[0, 2 * M + 1] == patch3d.AUG | patch3d.FLIP_W | patch3d.FLIP_D and t_on[0, 2 * M + 1] == t_off[0, 2 * M + 1] | patch3d.WARP
    assert t_on[1, 2 * M + 1] == t_off[1, 2 * M + 1] == patch3d.AUG                 # the item that drew no warp: flag clear,
    assert not t_on[1, 2 * M + 7:].any()                                            # and no matrix
    a = wchk.matrix(ang, zoom)
    assert (a < 0).any() and np.array_equal(t_on[0, 2 * M + 7:], wchk.pack(a))
    words = [int(v) & 0xffffffffffffffff for v in t_on[0, 2 * M + 7:]]
    got = [(words[e // 2] >> (32 * (e % 2))) & 0xffffffff for e in range(10)]
    assert [g - (1 << 32) if g >= 1 << 31 else g for g in got] == a.reshape(-1).tolist() + [0]
    assert patch3d.WARP == 64 and patch3d.WARP_EXTRA == 5 and patch3d.TABLE_EXTRA == 7
    txt = open(os.path.join(ROOT, 'include', 'mrdis.h')).read()
    assert int(re.search(r'#define\s+MRDIS_PATCH_WARP_FLAG\s+(\d+)', txt).group(1)) == patch3d.WARP
    assert hip.WARP_FAMILIES == ('patchwarp',) and 'patchwarp' in hip.LAUNCH_COUNTERS and 'patchwarp' in hip.launch_counts()
    assert hip.PATCH_FAMILIES == ('fgcount', 'patchorigin', 'patchgather')


# ---------------------------------------------------------------- the keys
def test_patch_warp_args_and_dataset_refusals():
    from mrdis import data3d
    assert data3d.patch_warp_args() == (0.0, (30.0, 30.0, 30.0), (0.7, 1.4))
    assert data3d.patch_warp_args(1, [0, 45, 7.5], [0.5, 2]) == (1.0, (0.0, 45.0, 7.5), (0.5, 2.0))
    assert data3d.patch_warp_args(0.3, (1, 2, 3), (1.0, 1.0))[2] == (1.0, 1.0)
    for bad in (-0.1, 1.01, '0.5', True, None, float('nan')):
        with pytest.raises(ValueError, match='patch_warp'):
            data3d.patch_warp_args(bad)
    for bad in ((30, 30), (30, 30, 46), (-1, 0, 0), 30, 'abc', (30, 30, True), (30, None, 30), (1, 2, float('inf'))):
        with pytest.raises(ValueError, match='patch_rot'):
            data3d.patch_warp_args(0.5, bad)
    for bad in ((0.7,), (1.4, 0.7), (0.4, 1.0), (1.0, 2.1), 1.0, 'ab', (0.7, 1.4, 1.5), (True, 1.4), (0.7, float('nan'))):
        with pytest.raises(ValueError, match='patch_zoom'):
            data3d.patch_warp_args(0.5, (30, 30, 30), bad)
    data, store = small_store()
    mk = lambda **kw: mrdis.VolumeDataset3D('BraTS', store, ['s0'], contrast_list=['T1'], aug=True, patch_size=(2, 2, 2), **kw)
    for key, bad in (('patch_warp', 2), ('patch_rot', (50, 0, 0)), ('patch_zoom', (2, 1))):
        with pytest.raises(ValueError, match=key):
            mk(**{key: bad})
        with pytest.raises(ValueError, match=key):
            mk().set_patch((2, 2, 2), **{key: bad})
        with pytest.raises(ValueError, match=key):
            mrdis.VolumeLoader3D(mk(), 1, patch_size=(2, 2, 2), **{key: bad})


def test_config_defaults_and_refusals():
    load = mrdis.train3d.load_config3d
    cfg = load(None, {})
    assert cfg['patch_warp'] == 0.0 and cfg['patch_rot'] == [30, 30, 30] and cfg['patch_zoom'] == [0.7, 1.4]
    yml = load(os.path.join(ROOT, 'config3d.yaml'))
    assert (yml['patch_warp'], yml['patch_rot'], yml['patch_zoom']) == (0.0, [30, 30, 30], [0.7, 1.4])
    assert load(None, {'patch_warp': 7, 'patch_rot': 'zz', 'patch_zoom': 3})['patch_size'] is None       # read only when patch_size is set
    cfg = load(None, {'patch_size': [16, 16, 16], 'patch_warp': '0.5', 'patch_rot': (10, 0, 45), 'patch_zoom': (1, 2)})
    assert cfg['patch_warp'] == 0.5 and cfg['patch_rot'] == [10.0, 0.0, 45.0] and cfg['patch_zoom'] == [1.0, 2.0]
    for key, bad in (('patch_warp', 1.5), ('patch_warp', -1), ('patch_rot', [30, 30]), ('patch_rot', [30, 30, 60]), ('patch_zoom', [1.4, 0.7]),
                     ('patch_zoom', [0.1, 1.0]), ('patch_zoom', 1.2)):
        with pytest.raises(ValueError, match=key):
            load(None, {'patch_size': [16, 16, 16], key: bad})
    with pytest.raises(KeyError):
        load(None, {'patch_twist': 1})


# ---------------------------------------------------------------- the binding's contract (the stub-library pattern of test_hip_contracts_cpu.py)
TAB = lambda B=2, M=4, extra=0: z(B, 2 * M + patch3d.TABLE_EXTRA + patch3d.WARP_EXTRA + extra, dtype=I64)
GEO = dict(M=4, shape=(5, 6, 7), patch=(2, 3, 4))
ROWS = {
    'patch_warp': (lambda: dict(table=TAB(), origins=z(2, 4, dtype=I32), **GEO), ['patch_warp'], [((2, 4, 2, 3, 4), F32), ((2, 4), F32)],
                   {'table dtype': to('table', I32), 'rows short': put('table', lambda: TAB(extra=-1)), 'rows of patch_gather': put('table', lambda: TAB(extra=-patch3d.WARP_EXTRA)),
                    'table not dense': strided('table'), 'table not 2-d': put('table', lambda: z(40, dtype=I64)), 'no sample': put('table', lambda: TAB(B=0)),
                    'origins dtype': to('origins', I64), 'origins short': short('origins'), 'origins narrow': put('origins', lambda: z(2, 3, dtype=I32)),
                    'origins not dense': strided('origins'), 'origins on another device': meta('origins'), 'patch larger than the volume': put('patch', lambda: (2, 3, 8)),
                    'K with the inputs': put('K', lambda: 3), 'M = 65': put('M', lambda: 65), 'volume of 2^31 voxels': put('shape', lambda: (2048, 1024, 1024))}),
    'patch_warp targets': (lambda: dict(table=TAB(), origins=z(2, 4, dtype=I32), targets=True, K=3, relabel=True, **GEO), ['patch_warp'], [((2, 3, 2, 3, 4), F32)],
                           {'K = 65': put('K', lambda: 65), 'K = -1': put('K', lambda: -1), 'K a float': put('K', lambda: 2.0), 'K a bool': put('K', lambda: True),
                            'rows short': put('table', lambda: TAB(extra=-1)), 'origins on another device': meta('origins')}),
    'patch_warp label': (lambda: dict(table=TAB(extra=3), origins=z(2, 4, dtype=I32), targets=True, **GEO), ['patch_warp'], [((2, 2, 3, 4), F32)],
                         {'origins long': put('origins', lambda: z(3, 4, dtype=I32))}),
}


def test_valid_calls_reach_the_entry_point(monkeypatch):
    stub = install_stub(monkeypatch.setattr)
    assert 'mrdis_patch_warp' in COMPUTE
    for name, (make, calls, shapes, _) in sorted(ROWS.items()):
        del stub.calls[:]
        result = patch3d.patch_warp(**make())
        assert stub.calls == calls, (name, stub.calls)
        assert [(tuple(t.shape), t.dtype) for t in tensors(result)] == [(tuple(s), d) for s, d in shapes], name
    x, mask = patch3d.patch_warp(**ROWS['patch_warp'][0]())
    assert x.permute(0, 2, 3, 4, 1).is_contiguous()                # channels-last-3d, what model3d reads


def test_mutated_calls_raise_before_any_entry_point(monkeypatch):
    stub = install_stub(monkeypatch.setattr)
    failures, n = [], 0
    for name, (make, _, _, mutations) in sorted(ROWS.items()):
        for what, mutate in mutations.items():
            kw = make()
            mutate(kw)
            del stub.calls[:]
            n += 1
            try:
                patch3d.patch_warp(**kw)
                how = 'no error'
            except hip.MrdisError:
                how = None
            except Exception as e:
                how = f'{type(e).__name__}: {e}'
            if how is not None or stub.calls:
                failures.append(f'{name} [{what}]: {how or "MrdisError"}; entry points reached: {stub.calls}')
    assert n >= 20 and not failures, '\n'.join(failures)


def test_binding_has_no_assert_statement():
    import ast
    tree = ast.parse(open(os.path.join(ROOT, 'representation-disentanglement_amd', 'warp3d.py')).read())
    assert not [n.lineno for n in ast.walk(tree) if isinstance(n, ast.Assert)]


def test_library_refuses_by_return_code():
    """the C entry point itself, on arguments it refuses before any launch (no GPU is touched): EINVAL / EUNSUPPORTED as mrdis_patch_gather,
    plus rows shorter than 2 M + 12"""
    lib = hip.load()
    M = 4
    tab, org, out = z(2, 2 * M + 12, dtype=I64), z(2, 4, dtype=I32), z(2 * 24 * M)
    call = lambda **kw: lib.mrdis_patch_warp(*[{**dict(table=tab.data_ptr(), ld=2 * M + 12, origins=org.data_ptr(), out=out.data_ptr(), mask=None, B=2, M=M, H=5, W=6, D=7,
                                                         PH=2, PW=3, PD=4, mode=0, K=0, relabel=0, stream=None), **kw}[k]
                                               for k in ('table', 'ld', 'origins', 'out', 'mask', 'B', 'M', 'H', 'W', 'D', 'PH', 'PW', 'PD', 'mode', 'K', 'relabel', 'stream')])
    EINVAL, EUNSUPPORTED = lib.mrdis_patch_gather(None, 0, None, None, None, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, None), call(B=65536)
    assert EINVAL < 0 and EUNSUPPORTED < 0 and EINVAL != EUNSUPPORTED
    for kw in (dict(ld=2 * M + 11), dict(ld=2 * M + 7), dict(table=None), dict(origins=None), dict(out=None), dict(B=0), dict(M=0), dict(M=65), dict(PD=8), dict(PH=0),
               dict(mode=2), dict(K=3), dict(mode=1, K=65), dict(mode=1, K=-1)):
        assert call(**kw) == EINVAL, kw
    assert call(H=2048, W=1024, D=1024) == EUNSUPPORTED
