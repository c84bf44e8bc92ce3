"""Patch sampling for the 3-D nets on the GPU (csrc/mrdis_patch.hip, patch3d.py, data3d.py's patch mode, Run3D with `patch_size`) against the
plain-numpy oracle tests/patch3d_check.py.  Every comparison is exact: integers for the tables and origins, bits for the gathered floats."""
import numpy as np
import pytest
import torch

import patch3d_check as chk
from fixtures_data3d import data3d_volumes, data3d_subjects

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
TOP = 2 ** 32 - 1
CLASSES = (1, 2, 4)


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


class Rows:
    """a gather table built by hand (include/mrdis.h), keeping alive the device tensors it points to"""

    def __init__(self, mrdis, M):
        self.p, self.M, self.rows, self.keep = mrdis.patch3d, M, [], []

    def add(self, vols, seg=None, prefix=None, fg=False, centre=False, u=(0, 0, 0, 0, 0), flips=(False, False, False), aug=False, scale=1.0, shift=0.0):
        """vols: M host arrays or None; seg: host array or None; prefix: True = build it on the device, None = pointer 0"""
        M, p = self.M, self.p
        row = np.zeros(2 * M + p.TABLE_EXTRA, dtype=np.int64)
        for m, v in enumerate(vols):
            if v is not None:
                t, mn = dev(v), dev(np.array([v.min()]))
                self.keep += [t, mn]
                row[m], row[M + m] = t.data_ptr(), mn.data_ptr()
        if seg is not None:
            t = dev(seg)
            self.keep.append(t)
            row[2 * M] = t.data_ptr()
            if prefix:
                pre = p.fg_prefix(t, CLASSES)
                self.keep.append(pre)
                row[2 * M + 3] = pre.data_ptr()
        row[2 * M + 1] = ((p.FLIP_H if flips[0] else 0) | (p.FLIP_W if flips[1] else 0) | (p.FLIP_D if flips[2] else 0) | (p.AUG if aug else 0)
                          | (p.FG if fg else 0) | (p.CENTRE if centre else 0))
        bits = np.array([scale, shift], np.float32).view(np.uint32).astype(np.uint64)
        w = np.array(u, dtype=np.uint64)
        row[2 * M + 2] = (bits[0] | (bits[1] << np.uint64(32))).view(np.int64)
        row[2 * M + 4] = (w[0] | (w[1] << np.uint64(32))).view(np.int64)
        row[2 * M + 5] = (w[2] | (w[3] << np.uint64(32))).view(np.int64)
        row[2 * M + 6] = w[4].view(np.int64)
        self.rows.append(row)

    def table(self):
        return torch.from_numpy(np.stack(self.rows)).to(DEV)


# ---------------------------------------------------------------- prefix tables
@pytest.mark.parametrize('shape', [(5, 7, 9), (8, 16, 24), (9, 11, 13)], ids=str)
def test_prefix_tables_equal_numpy_cumsum(mrdis, shape):
    """one partial block; exactly three blocks; a partial second block.  Class 2 is absent."""
    seg = np.random.RandomState(sum(shape)).choice([0, 1, 4, 3], size=shape).astype(np.float32)
    hip = mrdis.hip
    hip.launch_counts(reset=True)
    counts = mrdis.patch3d.fg_block_counts(dev(seg), CLASSES)
    c = hip.launch_counts()
    assert c['fgcount'] == 1 and c['all'] == 1, c
    want = chk.block_counts(seg, CLASSES)
    nblk = (seg.size + 1023) // 1024
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (nblk, 3) == want.shape
    np.testing.assert_array_equal(counts.cpu().numpy(), want)
    assert want[:, 1].sum() == 0 and want[:, 0].sum() > 0 and want[:, 2].sum() > 0
    prefix = mrdis.patch3d.fg_prefix(dev(seg), CLASSES).cpu().numpy()
    np.testing.assert_array_equal(prefix, np.concatenate([np.zeros((1, 3), np.int64), np.cumsum(want, axis=0)]))
    np.testing.assert_array_equal(prefix, chk.prefix_table(seg, CLASSES))
    assert prefix.dtype == np.int32 and prefix[-1].tolist() == [(seg == v).sum() for v in CLASSES]
    one = mrdis.patch3d.fg_block_counts(dev(seg), (4,)).cpu().numpy()
    np.testing.assert_array_equal(one[:, 0], want[:, 2])


# ---------------------------------------------------------------- origins
def _origins(mrdis, rows, shape, patch, classes=CLASSES):
    hip = mrdis.hip
    tab = rows.table()
    hip.launch_counts(reset=True)
    o = mrdis.patch3d.patch_origins(tab, rows.M, shape, patch, classes)
    c = hip.launch_counts()
    assert c['patchorigin'] == 1 and c['all'] == 1, c
    assert o.dtype == torch.int32 and tuple(o.shape) == (len(rows.rows), 4)
    return o.cpu().numpy()


def test_every_r_is_hit_by_its_u(mrdis):
    """41 foreground voxels of two classes (class 2 absent) over a two-block volume: for every class and every r, the draw u = ceil(r 2^32 / n)
    and the draw just below it"""
    shape, patch = (9, 11, 13), (4, 5, 6)
    rs = np.random.RandomState(5)
    seg = np.zeros(shape, np.float32)
    at = rs.choice(seg.size, 41, replace=False)
    seg.reshape(-1)[at[:25]] = 1
    seg.reshape(-1)[at[25:]] = 4
    vol = rs.randn(*shape).astype(np.float32)
    rows, want = Rows(mrdis, 1), []
    for ci, n in ((0, 25), (1, 16)):
        for r in range(n):
            for u_voxel in {chk.u_reaching(r, n), max(chk.u_reaching(r, n) - 1, 0)}:
                u = (chk.u_reaching(ci, 2), u_voxel, int(rs.randint(0, 2 ** 32)), int(rs.randint(0, 2 ** 32)), int(rs.randint(0, 2 ** 32)))
                rows.add([vol], seg, prefix=True, fg=True, u=u)
                want.append(chk.origin(shape, patch, u, fg=True, seg=seg, classes=CLASSES))
    got = _origins(mrdis, rows, shape, patch)
    np.testing.assert_array_equal(got, np.array([w[:4] for w in want]))
    assert set(got[:, 3].tolist()) == {0, 2}                                   # class indices in the list (1, 2, 4)
    flat = [np.flatnonzero(seg.reshape(-1) == v) for v in CLASSES]
    centres = {(w[3], (w[4][0] * 11 + w[4][1]) * 13 + w[4][2]) for w in want}
    assert centres == {(0, int(f)) for f in flat[0]} | {(2, int(f)) for f in flat[2]}       # every voxel of both classes was some row's centre
    for g, w in zip(got, want):
        assert all(g[a] <= w[4][a] < g[a] + patch[a] for a in range(3))


def test_block_border_corner_voxels_fallbacks_and_top_draw(mrdis):
    shape, patch = (8, 16, 24), (4, 6, 10)
    H, W, D = shape
    vol = np.random.RandomState(2).randn(*shape).astype(np.float32)
    border = np.zeros(shape, np.float32)
    border.reshape(-1)[[5, 1023, 1024, 2000]] = 1                              # the r-th voxel at the last index of block 0 and the first of block 1
    first, last, none = np.zeros(shape, np.float32), np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    first[0, 0, 0] = 2
    last[H - 1, W - 1, D - 1] = 4
    none[3, 3, 3] = 3                                                          # a label outside the class list: no present class
    rows, want = Rows(mrdis, 1), []

    def add(seg, u, fg=True, prefix=True, centre=False):
        rows.add([vol], seg, prefix=prefix, fg=fg, u=u, centre=centre)
        want.append(chk.origin(shape, patch, u, fg=fg, seg=seg, classes=CLASSES, has_prefix=bool(prefix), centre=centre))

    for r in range(4):
        add(border, (0, chk.u_reaching(r, 4), 1, 2, 3))
    add(first, (TOP, TOP, TOP, TOP, TOP))                                      # a single voxel at (0, 0, 0): the lower clamp on every axis
    add(last, (0, 0, 0, 0, 0))                                                 # ... at (H-1, W-1, D-1): the upper clamp on every axis
    uni = (123, 456, chk.u_reaching(3, 5), chk.u_reaching(7, 11), chk.u_reaching(14, 15))
    add(none, uni)                                                             # class absent
    add(None, uni)                                                             # target pointer 0
    add(border, uni, prefix=None)                                              # prefix pointer 0
    add(border, uni, fg=False)                                                 # not a foreground sample
    add(border, (TOP, TOP, TOP, TOP, TOP), fg=False)                           # u = 2^32 - 1 on every axis
    add(border, (0, 0, 0, 0, 0), fg=False)
    add(border, uni, centre=True)
    got = _origins(mrdis, rows, shape, patch)
    np.testing.assert_array_equal(got, np.array([w[:4] for w in want]))
    assert [w[4] for w in want[:4]] == [(0, 0, 5), (2, 10, 15), (2, 10, 16), (5, 3, 8)]
    assert got[4].tolist() == [0, 0, 0, 1] and got[5].tolist() == [H - 4, W - 6, D - 10, 2]
    assert all(got[i].tolist() == [3, 7, 14, -1] for i in (6, 7, 8, 9))
    assert got[10].tolist() == [H - 4, W - 6, D - 10, -1] and got[11].tolist() == [0, 0, 0, -1] and got[12].tolist() == [2, 5, 7, -1]
    # no class list at all: every sample takes the uniform rule
    np.testing.assert_array_equal(_origins(mrdis, rows, shape, patch, classes=())[:10, :3],
                                  np.array([chk.origin(shape, patch, [int(x) for x in _row_u(r)])[:3] for r in rows.rows[:10]]))
    # patch == volume: the only origin
    assert (_origins(mrdis, rows, shape, shape)[:, :3] == 0).all()


def _row_u(row):
    w = row[-3:].view(np.uint64)
    return (w[0] & np.uint64(TOP), w[0] >> np.uint64(32), w[1] & np.uint64(TOP), w[1] >> np.uint64(32), w[2] & np.uint64(TOP))


# ---------------------------------------------------------------- gather
def _volumes(M, shape, seed, positive=False):
    rs = np.random.RandomState(seed)
    vols = []
    for m in range(M):
        v = rs.randn(*shape).astype(np.float32)
        if positive:
            v = np.abs(v) + 1
        else:
            v[rs.rand(*shape) < 0.3] = -10.0                                   # the z-score files' background marker
        vols.append(v)
    seg = rs.randint(0, 5, size=shape).astype(np.float32)
    return vols, seg


def _check_gather(mrdis, M, shape, patch, items, K=3, forms=(0, 1)):
    """items: dicts(vols, seg, origin, flips, aug, scale, shift).  Inputs, mask, label targets and K region channels of both forms of the kernel
    against the oracle, to the bit."""
    hip, p = mrdis.hip, mrdis.patch3d
    rows = Rows(mrdis, M)
    for it in items:
        rows.add(it['vols'], it.get('seg'), flips=it.get('flips', (False,) * 3), aug=it.get('aug', False), scale=it.get('scale', 1.0), shift=it.get('shift', 0.0))
    tab = rows.table()
    origins = dev(np.array([tuple(it['origin']) + (-1,) for it in items]), np.int32)
    want_x, want_m, want_t, want_k = [], [], [], []
    for it in items:
        x, m = chk.gather_inputs(it['vols'], it['origin'], patch, it.get('flips', (False,) * 3), it.get('aug', False), it.get('scale', 1.0), it.get('shift', 0.0))
        want_x.append(x); want_m.append(m)
        want_t.append(chk.gather_targets(it.get('seg'), it['origin'], patch, it.get('flips', (False,) * 3), 0))
        want_k.append(chk.gather_targets(it.get('seg'), it['origin'], patch, it.get('flips', (False,) * 3), K))
    out = None
    for gen in forms:
        hip.set_option('debug_volgen', gen)
        hip.launch_counts(reset=True)
        x, mask = p.patch_gather(tab, origins, M, shape, patch)
        t = p.patch_gather(tab, origins, M, shape, patch, targets=True, relabel=True)
        k = p.patch_gather(tab, origins, M, shape, patch, targets=True, K=K, relabel=True)
        c = hip.launch_counts()
        assert c['patchgather'] == 3 and c['all'] == 3 and c['volgather'] == 0, c
        assert x.permute(0, 2, 3, 4, 1).is_contiguous() and k.permute(0, 2, 3, 4, 1).is_contiguous()
        np.testing.assert_array_equal(x.cpu().numpy(), np.stack(want_x))
        np.testing.assert_array_equal(mask.cpu().numpy(), np.stack(want_m))
        np.testing.assert_array_equal(t.cpu().numpy(), np.stack(want_t))
        np.testing.assert_array_equal(k.cpu().numpy(), np.stack(want_k))
        out = x
    hip.set_option('debug_volgen', 0)
    return out, rows, origins            # (`rows` owns the device volumes the table points to)


FLIPS = [(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)]


def test_gather_m4_all_flips_and_corners(mrdis):
    """M = 4 (the specialised tile): the eight flip combinations, each at one of the eight corner origins, augmented, with an absent contrast in
    some items; 4 * 6 * 8 * 4 floats per item: one partial tile"""
    shape, patch = (10, 12, 14), (4, 6, 8)
    vols, seg = _volumes(4, shape, 1)
    corners = [(h, w, d) for h in (0, 6) for w in (0, 6) for d in (0, 6)]
    items = [dict(vols=[v if (m != i % 4 or i < 4) else None for m, v in enumerate(vols)], seg=seg, origin=corners[i], flips=FLIPS[i], aug=True,
                  scale=0.9 + 0.025 * i, shift=-0.1 + 0.03 * i) for i in range(8)]
    items += [dict(vols=vols, seg=seg, origin=corners[7 - i], flips=FLIPS[i]) for i in range(8)]       # not augmented: the raw values
    x, _, _ = _check_gather(mrdis, 4, shape, patch, items)
    assert int((x == -10).sum()) > 0


def test_gather_runtime_tile_odd_depth_and_element_form(mrdis):
    """M = 3 (the run-time tile) with PD = 6 and PD = 5 (no multiple of 4), origins at odd offsets; M = 5 with patch (3, 3, 3): 135 floats per
    item, no multiple of 4 -> the element form under the default policy too; M = 8 / 16 (the padded tiles)"""
    for M, shape, patch, seed in ((3, (7, 9, 11), (4, 5, 6), 2), (3, (7, 9, 11), (4, 4, 5), 3), (5, (5, 6, 7), (3, 3, 3), 4), (8, (6, 7, 9), (3, 5, 7), 5),
                                  (16, (4, 6, 9), (2, 4, 6), 6), (33, (3, 4, 6), (2, 2, 4), 7)):
        vols, seg = _volumes(M, shape, seed)
        items = [dict(vols=vols, seg=seg if i != 2 else None, origin=tuple(int(v) for v in np.random.RandomState(seed + i).randint(0, np.array(shape) - patch + 1)),
                      flips=FLIPS[(3 * i + seed) % 8], aug=i % 2 == 0, scale=1.07, shift=0.04) for i in range(3)]
        _check_gather(mrdis, M, shape, patch, items)


def test_gather_partial_last_tile(mrdis):
    """PH PW PD = 1200 at M = 4: a tile of 1024 positions and a partial one of 176; B = 2"""
    shape, patch = (11, 12, 13), (10, 10, 12)
    vols, seg = _volumes(4, shape, 8)
    items = [dict(vols=vols, seg=seg, origin=(1, 2, 1), flips=(True, False, True), aug=True, scale=1.1, shift=0.1),
             dict(vols=vols, seg=seg, origin=(0, 0, 0), flips=(False, True, False))]
    _check_gather(mrdis, 4, shape, patch, items)


def test_gather_absent_and_dropped_contrasts_and_the_minimum_rule(mrdis):
    """an absent contrast reads as zeros with mask 0.  With positive volumes m0 falls to 0, so exactly the absent contrast's zeros become -10;
    with a -10 background m0 = -10: the background becomes -10 and the absent contrast's zeros become `shift`.  m0 is the minimum of the
    whole stored volumes: a patch without background keeps its own minimum."""
    shape, patch = (6, 8, 10), (3, 4, 4)
    pos, seg = _volumes(4, shape, 9, positive=True)
    items = [dict(vols=[pos[0], None, pos[2], None], seg=seg, origin=(1, 2, 3), aug=True, scale=1.05, shift=0.07, flips=(False, True, False))]
    x, _, _ = _check_gather(mrdis, 4, shape, patch, items)
    x = x.cpu().numpy()
    assert (x[0, 1] == -10).all() and (x[0, 3] == -10).all() and (x[0, 0] > 0).all() and (x[0, 2] > 0).all()
    bg, _ = _volumes(4, shape, 10)
    for v in bg:
        v[1:4, 2:6, 3:7] = np.abs(v[1:4, 2:6, 3:7]) + 1                        # this patch holds no background voxel
    items = [dict(vols=[bg[0], None, bg[2], bg[3]], seg=None, origin=(1, 2, 3), aug=True, scale=1.05, shift=0.07),
             dict(vols=[bg[0], None, bg[2], bg[3]], seg=None, origin=(0, 0, 0), aug=True, scale=1.05, shift=0.07)]
    x, _, _ = _check_gather(mrdis, 4, shape, patch, items)
    x = x.cpu().numpy()
    assert not (x[0] == -10).any() and (x[0, 1] == np.float32(0.07)).all() and (x[1] == -10).any()


def test_whole_volume_patch_equals_volume_gather(mrdis):
    """patch == volume, no flip: the bits of hip.volume_gather(z0=0, Dz=D) over the same table (its first 2 M + 3 words are that kernel's)"""
    shape = (6, 10, 12)
    vols, seg = _volumes(4, shape, 11)
    items = [dict(vols=vols, seg=seg, origin=(0, 0, 0), aug=True, scale=0.93, shift=-0.05), dict(vols=[vols[0], None, vols[1], vols[2]], seg=seg, origin=(0, 0, 0))]
    x, rows, origins = _check_gather(mrdis, 4, shape, shape, items, forms=(0,))
    tab = rows.table()
    H, W, D = shape
    wx, wmask = mrdis.hip.volume_gather(tab, 4, H, W, D, 0, D)
    wt = mrdis.hip.volume_gather(tab, 4, H, W, D, 0, D, targets=True, K=3, relabel=True)
    gx, gmask = mrdis.patch3d.patch_gather(tab, origins, 4, shape, shape)
    gt = mrdis.patch3d.patch_gather(tab, origins, 4, shape, shape, targets=True, K=3, relabel=True)
    assert torch.equal(gx, wx) and torch.equal(gmask, wmask) and torch.equal(gt, wt) and torch.equal(gx, x)
    assert gx.stride() == wx.stride()
    # origins outside the volume are clamped into it by the kernel: nothing is read past the border
    far = dev(np.array([[99, -5, 7, -1], [-1, 99, 99, -1]]), np.int32)
    assert torch.equal(mrdis.patch3d.patch_gather(tab, far, 4, shape, shape)[0], wx)


def test_three_entry_points_agree_bit_for_bit(mrdis):
    """volume_gather (z0 = 0, Dz = D), patch_gather of the whole volume at origin 0 and patch_warp with the WARP flag clear (its rows carry a
    matrix all the same) are one gather: the same bits for the inputs, the mask, the label targets and K = 3 region channels, as dispatched
    and under debug_volgen, one launch of the entry point's own family per call.  (9, 10, 13): 1170 positions, two flat tiles with the second
    partial at M = 4 (the CM = 4 tile); M = 3 (M at run time) and every target leave no multiple of four floats: the element kernel by itself.
    Rows: plain, H flip, augmented, both with the second contrast absent."""
    hip, p = mrdis.hip, mrdis.patch3d
    shape = H, W, D = (9, 10, 13)
    vols, seg = _volumes(4, shape, 12)
    matrix = torch.from_numpy(p.pack_warp(p.warp_matrix((10.0, -20.0, 30.0), 1.2))).to(DEV)
    origins = torch.zeros((4, 4), dtype=torch.int32, device=DEV)
    before = hip.get_option('debug_volgen')
    try:
        for M in (4, 3):
            rows = Rows(mrdis, M)
            for i, (flip, aug) in enumerate(((False, False), (True, False), (False, True), (True, True))):
                rows.add([v if (i, m) != (3, 1) else None for m, v in enumerate(vols[:M])], seg, flips=(flip, False, False), aug=aug, scale=1.06, shift=-0.03)
            tab = rows.table()
            warp_tab = torch.cat([tab, matrix.expand(4, -1)], dim=1).contiguous()
            assert warp_tab.shape[1] == 2 * M + p.TABLE_EXTRA + p.WARP_EXTRA and not (tab[:, 2 * M + 1] & p.WARP).any()
            for gen in (0, 1):
                hip.set_option('debug_volgen', gen)
                for kw in ({}, dict(targets=True, K=0, relabel=True), dict(targets=True, K=3, relabel=True)):
                    got = []
                    for family, call in (('volgather', lambda: hip.volume_gather(tab, M, H, W, D, 0, D, **kw)),
                                         ('patchgather', lambda: p.patch_gather(tab, origins, M, shape, shape, **kw)),
                                         ('patchwarp', lambda: p.patch_warp(warp_tab, origins, M, shape, shape, **kw))):
                        hip.launch_counts(reset=True)
                        out = call()
                        c = hip.launch_counts()
                        assert c[family] == 1 and c['all'] == 1, (family, M, gen, kw, c)
                        got.append(out if isinstance(out, tuple) else (out,))
                    for family, other in zip(('patchgather', 'patchwarp'), got[1:]):
                        assert len(other) == len(got[0]), (family, M, gen, kw)
                        for a, b in zip(got[0], other):
                            assert a.shape == b.shape and a.stride() == b.stride() and torch.equal(a.view(torch.int32), b.view(torch.int32)), (family, M, gen, kw)
                    if not kw:                                         # the rows are what they claim to be: a flip, a marker, an absent contrast
                        x, mask = got[0]
                        assert torch.equal(x[1], x[0].flip(1)) and int((x[2] == -10).sum()) > 0 and mask.tolist() == [[1.0] * M] * 3 + [[1.0, 0.0] + [1.0] * (M - 2)]
    finally:
        hip.set_option('debug_volgen', before)


# ---------------------------------------------------------------- the loader
CONTRASTS = ['T1', 'T1c', 'T2', 'T2_FLAIR']


@pytest.fixture(scope='module')
def loader_world():
    data = data3d_volumes(n_subj=5, H=12, W=16, D=24, contrasts=CONTRASTS, seed=13)
    for k in [k for k in data if k.endswith('/seg')]:                          # sparse tumours: most patches would miss them by chance
        seg = np.zeros_like(data[k])
        rs = np.random.RandomState(len(k) + int(k[-7:-4]))
        seg.reshape(-1)[rs.choice(seg.size, 12, replace=False)] = rs.choice([1, 2, 4], 12)
        data[k] = seg
    return data, data3d_subjects(data)


def _patch_loader(mrdis, world, **kw):
    data, subj = world
    store = mrdis.VolumeStore3D.from_arrays(data, DEV)
    args = dict(aug=True, dropoff=True)
    args.update({k: kw.pop(k) for k in ('aug', 'dropoff') if k in kw})
    ds = mrdis.VolumeDataset3D('BraTS', store, subj, CONTRASTS, **args)
    return mrdis.VolumeLoader3D(ds, 2, shuffle=False, region_channels=kw.pop('K', 3), **kw)


def test_seeded_loader_gives_the_oracles_batches(mrdis, loader_world):
    """patch_fg = 1: every item is centred on a tumour voxel, and every patch contains it -- the property that shows the oversampling happened"""
    data, subj = loader_world
    patch = (8, 8, 16)
    la = _patch_loader(mrdis, loader_world, patch_size=patch, patch_fg=1.0, patch_flips='hwd')
    n = 0
    for epoch in range(2):
        np.random.seed(31 + epoch)
        got = list(la)
        want = chk.loader_batches(data, subj, CONTRASTS, 2, patch, np.random.RandomState(31 + epoch), aug=True, dropoff=True, patch_fg=1.0, patch_flips='hwd', K=3)
        assert len(got) == len(want) == 3
        twin = np.random.RandomState(31 + epoch)
        chk.loader_batches(data, subj, CONTRASTS, 2, patch, twin, aug=True, dropoff=True, patch_fg=1.0, patch_flips='hwd', K=3)
        assert np.random.get_state()[2] == twin.get_state()[2] and (np.random.get_state()[1] == twin.get_state()[1]).all()     # the same draws, no more
        for b, w in zip(got, want):
            assert b['inputs'].shape == (len(w['inputs']), 4) + patch and b['inputs'].permute(0, 2, 3, 4, 1).is_contiguous()
            np.testing.assert_array_equal(b['origins'].cpu().numpy(), w['origins'])
            np.testing.assert_array_equal(b['inputs'].cpu().numpy(), w['inputs'])
            np.testing.assert_array_equal(b['targets'].cpu().numpy(), w['targets'])
            np.testing.assert_array_equal(b['mask'].cpu().numpy(), w['mask'])
            np.testing.assert_array_equal(b['mask_host'], w['mask'])
            for o, centre in zip(w['origins'], w['centres']):
                assert o[3] >= 0 and all(o[a] <= centre[a] < o[a] + patch[a] for a in range(3))
                n += 1
    assert n == 10
    # the evaluation form: the centre patch, no draw but the drop-off's
    ev = _patch_loader(mrdis, loader_world, aug=False, patch_size=patch, patch_centre=True)
    np.random.seed(5)
    got = list(ev)
    want = chk.loader_batches(data, subj, CONTRASTS, 2, patch, np.random.RandomState(5), dropoff=True, K=3, centre=True)
    for b, w in zip(got, want):
        assert b['origins'].cpu().tolist() == [[2, 4, 4, -1]] * len(w['inputs'])
        np.testing.assert_array_equal(b['inputs'].cpu().numpy(), w['inputs'])
        np.testing.assert_array_equal(b['targets'].cpu().numpy(), w['targets'])
    assert ev.dataset.crop() == (4, 16)


def test_launch_counters_per_batch(mrdis, loader_world):
    hip = mrdis.hip
    la = _patch_loader(mrdis, loader_world, patch_size=(8, 8, 16), patch_fg=1.0)
    np.random.seed(1)
    list(la)                                                                   # the prefix tables and minima are made once, before the counted region
    hip.launch_counts(reset=True)
    n = len(list(la))
    c = hip.launch_counts()
    assert n == 3 and c['patchorigin'] == n and c['patchgather'] == 2 * n and c['volgather'] == 0 and c['fgcount'] == 0 and c['all'] == 3 * n, c
    data = data3d_volumes(n_subj=3, H=8, W=8, D=99, contrasts=CONTRASTS, seed=1)
    store = mrdis.VolumeStore3D.from_arrays(data, DEV)
    plain = mrdis.VolumeLoader3D(mrdis.VolumeDataset3D('BraTS', store, data3d_subjects(data), CONTRASTS, aug=True), 2, region_channels=3)
    assert plain.dataset.patch_size is None
    list(plain)
    hip.launch_counts(reset=True)
    n = len(list(plain))
    c = hip.launch_counts()
    assert n == 2 and c['volgather'] == 2 * n and c['all'] == 2 * n and not any(c[f] for f in hip.PATCH_FAMILIES), c
    assert 'origins' not in next(iter(plain))


def test_three_launches_replay_through_a_graph_with_the_next_table(mrdis, loader_world):
    data, subj = loader_world
    patch = (8, 8, 16)
    la = _patch_loader(mrdis, loader_world, patch_size=patch, patch_fg=0.5, patch_flips='hwd')
    ds, st = la.dataset, la.dataset.store
    p = mrdis.patch3d
    np.random.seed(41)
    plans = [pl for _ in range(2) for pl in la.batch_plan() if len(pl[2]) == 2]
    tabs = [torch.from_numpy(la.patch_table(m)[0]).to(DEV) for _, _, m in plans]           # (builds the prefix tables and minima)
    assert len(tabs) == 4 and not torch.equal(tabs[0], tabs[1])
    static = tabs[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        o = p.patch_origins(static, 4, st.shape, patch, CLASSES)                          # warm-up outside the capture
        p.patch_gather(static, o, 4, st.shape, patch)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o = p.patch_origins(static, 4, st.shape, patch, CLASSES)
        x, mask = p.patch_gather(static, o, 4, st.shape, patch)
        t = p.patch_gather(static, o, 4, st.shape, patch, targets=True, K=3, relabel=True)
    np.random.seed(41)
    want = [w for _ in range(2) for w in chk.loader_batches(data, subj, CONTRASTS, 2, patch, np.random, aug=True, dropoff=True, patch_fg=0.5, patch_flips='hwd', K=3)
            if len(w['inputs']) == 2]
    for tab, w in zip(tabs, want):
        static.copy_(tab)
        g.replay()
        np.testing.assert_array_equal(o.cpu().numpy(), w['origins'])
        np.testing.assert_array_equal(x.cpu().numpy(), w['inputs'])
        np.testing.assert_array_equal(t.cpu().numpy(), w['targets'])
        np.testing.assert_array_equal(mask.cpu().numpy(), w['mask'])
    assert {int(v) for w in want for v in w['origins'][:, 3]} > {-1}           # both rules were replayed


# ---------------------------------------------------------------- Run3D
@pytest.fixture(scope='module')
def run_world(tmp_path_factory):
    data = data3d_volumes(n_subj=11, H=32, W=48, D=40, contrasts=CONTRASTS, seed=17)
    subj = data3d_subjects(data)
    root = tmp_path_factory.mktemp('patch3d')
    for name, part in (('train', subj[:5]), ('val', subj[5:8]), ('test', subj[8:11])):
        (root / f'fold_BraTS_3d_0_{name}_noval.txt').write_text('\n'.join(part) + '\n')
    return data, str(root), subj


def _run(mrdis, world, ckpt, **over):
    cfg = dict(dataset_name='BraTS', data_path=world[1], contrast_list=CONTRASTS, batch_size=2, model_name='NVNet3D', init_channels=8, epochs=2, lr=1e-4,
               ckpt_path=str(ckpt), device='cuda:0', seed=10, patch_size=[16, 16, 16], patch_fg=0.5, patch_flips='hwd')
    cfg.update(over)
    return mrdis.Run3D(cfg, store=mrdis.VolumeStore3D.from_arrays(world[0], DEV), log=lambda *a: None)


def test_run3d_trains_resumes_and_predicts_on_patches(mrdis, run_world, tmp_path):
    hip = mrdis.hip
    straight = _run(mrdis, run_world, tmp_path / 'straight')
    assert straight.input_shape == (16, 16, 16) and straight.loaders['train'].dataset.patch_fg == 0.5
    assert straight.loaders['val'].dataset.patch_centre and straight.loaders['val'].dataset.patch_fg == 0.0 and not straight.loaders['train'].dataset.patch_centre
    hip.launch_counts(reset=True)
    straight.train()
    c = hip.launch_counts()
    steps, vals = len(straight.loaders['train']), len(straight.loaders['val'])
    assert steps == 2 and vals == 1                                            # two training batches and a validation pass per epoch
    assert c['patchorigin'] == 2 * (steps + vals) and c['patchgather'] == 4 * (steps + vals) and c['volgather'] == 0, c
    assert 0 < straight.last_stat['dice'] < 1 and np.isfinite(straight.last_stat['loss'])
    first = _run(mrdis, run_world, tmp_path / 'resumed')
    first._train(1)                                                            # an interrupted run
    del first
    second = _run(mrdis, run_world, tmp_path / 'resumed', continue_train=True)
    assert second.start_epoch == 0
    second.train()
    a, b = straight.model.state_dict(), second.model.state_dict()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert straight.last_stat == second.last_stat
    # phase predict: the trained depth 16 slides over the full 32 x 48 planes at depth offsets 0, 8, 16, 24
    assert mrdis.window_offsets(40, 16, 8) == [0, 8, 16, 24]
    pred = _run(mrdis, run_world, tmp_path / 'straight', phase='predict')
    assert pred.loaders['test'].dataset.crop() == (12, 16)
    hip.launch_counts(reset=True)
    pred.predict()
    c = hip.launch_counts()
    assert c['segaccum'] == 4 and c['volgather'] == 8 and not any(c[f] for f in hip.PATCH_FAMILIES), c      # per window: inputs and targets
    out = tmp_path / 'straight' / 'result_test'
    for sid in run_world[2][9:11]:                                             # (the list reader takes the first line as a header)
        lab = np.load(out / f'{sid}_seg.npy')
        assert lab.shape == (32, 48, 40) and lab.dtype == np.uint8 and set(np.unique(lab)) <= {0, 1, 2, 4}
