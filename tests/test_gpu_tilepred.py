"""Tile-wise prediction on the GPU: the two kernels of csrc/mrdis_segvol.hip behind tilepred.tile_accum / tilepred.tile_label_volume,
model3d.predict_tiles, VolumeLoader3D.tile and `Run3D` with `predict_tile`, against the float64 oracle tests/tilepred_check.py.

Which shape takes which kernel path (header of mrdis_segvol.hip: a lane owns one ALIGNED group of four acc floats / four voxels; groups cut by
the start or end of a run / a sample go element by element; a view that mirrors d reads its logits by element loads, every other view by one
16-byte load per group):
  main      B 2, C 3, 9 x 10 x 37, tile 6 x 8 x 16 at strides 3, 4, 8: an acc column is 111 floats and the run of a tile column starts
            3 (37 col + d0) floats in, d0 in 0 8 16 21 -- every alignment phase occurs in every launch: vector groups inside the runs, element
            groups at both ends.  H W D = 3330, % 4 = 2: sample 1 starts inside a group of the label kernel, and columns end inside groups
            (37 % 4 = 1), so the (h, w) product of the denominator is formed again inside a group.  Views '', h, wd, hwd: both load forms.
  c1        B 3, C 1, same geometry: a run is 16 floats at phase (37 col + d0) % 4; samples start at voxel phases 0, 2, 0.
  elements  B 1, C 1, 3 x 5 x 7, tile 2 x 3 x 3: a run of 3 floats never fills a group -- the accumulation's element path alone, plain and
            d-mirrored; H W D = 105: the label kernel's last group is partial.
  vectors   B 2, C 4, 4 x 6 x 16, tile 4 x 4 x 8 at d0 0 8: every run starts and ends on a group boundary and H W D % 4 == 0 -- the vector
            paths alone (C = 4: a voxel is a group).
  allviews  B 1, C 3, 6 x 6 x 10, tile 4 x 4 x 8, stride 2: all eight views on every tile, 2 x 2 x 2 tiles.

Tolerances.  The accumulation has none fixed in advance: max |acc - acc64| / den of the fp32 torch composition of the same rule (torch.sigmoid,
the same fp32 weight product, += in the same order, on the device) is measured in the same test, and the kernel may be at most twice as far
off.  Labels and counts may differ from the float64 oracle only at EXCUSED voxels: some |pbar_c - 0.5|, or the gap of the two largest pbar, below
8 (n_acc + 1) 2^-24 with n_acc the largest number of accumulations on a voxel of the run (tilepred_check.excuse_bound).  At most 1e-3 of a
case's voxels may be excused, counted over the view sets the case runs with and asserted from the oracle alone before any kernel output is
looked at.  With seed 12, Gaussian weights of sigma 0.125 and this file's draw order (logits per (tile, view) in launch order, then the label
volumes) the excused counts per view set are: main 0 + 4 + 5 + 10 of 4 x 6660 (n_acc 12, 24, 48, 96: the bound and so the count grow with the
views), c1 0 + 2 + 1 + 2 of 4 x 9990, elements 0, vectors 0, allviews 0."""
import os

import numpy as np
import pytest
import torch

import tilepred_check as T
from fixtures_data3d import data3d_volumes, data3d_subjects

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
KINDS = ('gaussian', 'uniform', 'random')


# ----------------------------------------------------------------------------------------------- helpers
def dev_weights(w):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in w)


def run_kernels(mrdis, c, geom=None, logits=None, relabel=False, tvol='own'):
    """the kernels on the device: acc, labels, counts, all back on the CPU"""
    tp = mrdis.tilepred
    geom = c['geom'] if geom is None else geom
    logits = c['logits'] if logits is None else logits
    acc = torch.zeros(c['B'], *c['shape'], c['C'], device=DEV)
    w = dev_weights(c['w'])
    for (origin, v), l in zip(geom, logits):
        tp.tile_accum(l.to(DEV).permute(0, 4, 1, 2, 3), acc, w, origin, v)
    vols = ptrs = None
    if tvol is not None:
        vols = [x.contiguous().to(DEV) for x in c['tvol']]
        ptrs = torch.tensor([x.data_ptr() for x in vols], dtype=torch.int64).to(DEV)
    labels, counts = tp.tile_label_volume(acc, dev_weights(c['norms']), ptrs, relabel=relabel)
    torch.cuda.synchronize()
    del vols
    return acc.cpu(), labels.cpu(), counts.cpu()


def torch_composition(c):
    """the fp32 torch composition of the rule on the device, in launch order: (B, H, W, D, C) on the CPU"""
    TH, TW, TD = c['tile']
    wh, ww, wd = dev_weights(c['w'])
    w3 = ((wh[:, None] * ww[None, :])[:, :, None] * wd[None, None, :])[None, ..., None]         # (wh ww) wd: two fp32 roundings
    acc = torch.zeros(c['B'], *c['shape'], c['C'], device=DEV)
    for ((h0, w0, d0), v), l in zip(c['geom'], c['logits']):
        p = torch.sigmoid(l.to(DEV))
        dims = [a for a, bit in ((1, T.FLIP_H), (2, T.FLIP_W), (3, T.FLIP_D)) if v & bit]
        if dims:
            p = p.flip(dims)
        acc[:, h0:h0 + TH, w0:w0 + TW, d0:d0 + TD] += w3 * p
    return acc.cpu()


# ----------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize('name,mirror', T.CASE_VIEWS)
def test_accumulation_within_twice_the_torch_error_of_float64(mrdis, name, mirror):
    for kind in KINDS:
        c = T.make_case(name, mirror, kind)
        acc64, den64, n_acc = T.oracle_acc(c)
        assert float(den64.min()) > 0
        d = den64[None, ..., None]
        acc, _, _ = run_kernels(mrdis, c, tvol=None)
        e_torch = float((np.abs(torch_composition(c).double().numpy() - acc64) / d).max())
        e_kernel = float((np.abs(acc.double().numpy() - acc64) / d).max())
        print(f'\n[tilepred accum {name} {mirror!r} {kind}] max |acc - float64| / den: kernel {e_kernel:.3e}  torch fp32 composition {e_torch:.3e}  '
              f'(n_acc {int(n_acc.max())}, {len(c["geom"])} launches)')
        assert e_torch > 0
        assert e_kernel <= 2 * e_torch


def test_acc_stays_zero_where_no_tile_reaches(mrdis):
    c = T.make_case('main', 'hwd')
    keep = [i for i, (o, v) in enumerate(c['geom']) if o in ((0, 0, 0), (3, 2, 8))]              # two tiles that overlap, all eight views
    geom, logits = [c['geom'][i] for i in keep], [c['logits'][i] for i in keep]
    _, _, n_acc = T.oracle_acc(c, geom, logits)
    assert int((n_acc == 0).sum()) > 0 and int((n_acc == 16).sum()) > 0                           # untouched voxels, and the tiles' overlap
    acc, _, _ = run_kernels(mrdis, c, geom, logits, tvol=None)
    assert float(acc[:, torch.from_numpy(n_acc == 0)].abs().max()) == 0.0
    assert float(acc[:, torch.from_numpy(n_acc > 0)].min()) > 0.0


@pytest.mark.parametrize('name', list(T.CASES))
def test_labels_and_counts_against_the_float64_oracle(mrdis, name):
    runs = []
    for mirror in T.CASES[name]['mirrors']:
        c = T.make_case(name, mirror)
        acc64, den64, n_acc = T.oracle_acc(c)
        runs.append((c, T.oracle_labels(acc64, den64, c['tvol'], False, T.excuse_bound(n_acc.max()))))
    # conditions on the inputs, from the oracle alone
    n_exc, n_vox = sum(int(r[3].sum()) for _, r in runs), sum(r[3].size for _, r in runs)
    print(f'\n[tilepred labels {name}] excused per view set {[int(r[3].sum()) for _, r in runs]} of {runs[0][1][3].size} each')
    assert n_exc <= T.EXCUSED_SHARE * n_vox, (n_exc, n_vox)
    for c, (want, pred, lab, excused) in runs:
        assert len(set(want.flatten().tolist())) == c['C'] + 1                                    # every label occurs
    for c, (want, pred, lab, excused) in runs:
        _, labels, counts = run_kernels(mrdis, c)
        assert labels.dtype == torch.uint8 and tuple(labels.shape) == (c['B'], *c['shape'])
        assert counts.dtype == torch.int32 and tuple(counts.shape) == (c['B'], c['C'], 3)
        what = f'{name} {c["mirror"]!r}'
        bad = (labels.numpy().astype(np.int64) != want) & ~excused
        assert int(bad.sum()) == 0, f'{what}: {int(bad.sum())} labels differ outside the excused voxels'
        lo = T.counts_of(pred, lab, ~excused)
        hi = lo + excused.reshape(excused.shape[0], -1).sum(1)[:, None, None]
        got = counts.numpy().astype(np.int64)
        assert bool(((got >= lo) & (got <= hi)).all()), f'{what}: counts {got.tolist()} outside [{lo.tolist()}, {hi.tolist()}]'
        assert np.array_equal(got[..., 2], T.counts_of(pred, lab, np.ones_like(excused))[..., 2]), what


def test_relabel_and_missing_targets(mrdis):
    c = T.make_case('main', 'h', labels_max=4)
    c['tvol'][c['tvol'] == 3] = 4                                                                # BraTS raw labels: 0 / 1 / 2 / 4
    acc64, den64, n_acc = T.oracle_acc(c)
    want, pred, lab, excused = T.oracle_labels(acc64, den64, c['tvol'], True, T.excuse_bound(n_acc.max()))
    assert int(excused.sum()) <= T.EXCUSED_SHARE * excused.size
    _, labels, counts = run_kernels(mrdis, c, relabel=True)
    T.assert_labels_counts(labels, counts, want, pred, lab, excused, 'relabel')
    assert set(labels.flatten().tolist()) == {0, 1, 2, 4}
    assert int(counts[:, 2, 2].sum()) == int((c['tvol'] == 4).sum()) > 0                         # a 4 in the target counts under channel 2
    _, labels_n, counts_n = run_kernels(mrdis, c, relabel=True, tvol=None)                       # no targets at all
    assert torch.equal(labels_n, labels) and int(counts_n[:, :, [0, 2]].abs().sum()) == 0 and torch.equal(counts_n[:, :, 1], counts[:, :, 1])


def test_whole_plane_tiles_with_unit_weights_are_seg_accum_to_the_bit(mrdis):
    hip, tp = mrdis.hip, mrdis.tilepred
    B, C, H, W, D, Dz = 2, 3, 9, 10, 37, 16
    g = torch.Generator().manual_seed(T.SEED)
    ones = tuple(torch.ones(n, device=DEV) for n in (H, W, Dz))
    a_tile, a_seg = torch.zeros(B, H, W, D, C, device=DEV), torch.zeros(B, H, W, D, C, device=DEV)
    for z0 in (0, 8, 16, 21):
        for f in (False, True):
            l = (3 * torch.randn(B, H, W, Dz, C, generator=g)).to(DEV).permute(0, 4, 1, 2, 3)
            tp.tile_accum(l, a_tile, ones, (0, 0, z0), T.FLIP_H if f else 0)
            hip.seg_accum(l, a_seg, z0, flip_h=f)
    assert torch.equal(a_tile, a_seg) and float(a_seg.max()) > 2
    # the label kernel: nh = nw = 1, nd = cover
    cover = torch.zeros(D, dtype=torch.int32)
    for z0 in (0, 8, 16, 21):
        cover[z0:z0 + Dz] += 2
    tvol = [torch.randint(0, 5, (H, W, D), generator=g).float().to(DEV) for _ in range(B)]
    ptrs = torch.tensor([v.data_ptr() for v in tvol], dtype=torch.int64).to(DEV)
    for relabel in (False, True):
        l_seg, c_seg = hip.seg_label_volume(a_seg, cover.to(DEV), ptrs, relabel=relabel)
        l_tile, c_tile = tp.tile_label_volume(a_tile, (torch.ones(H, device=DEV), torch.ones(W, device=DEV), cover.float().to(DEV)), ptrs, relabel=relabel)
        assert torch.equal(l_seg, l_tile) and torch.equal(c_seg, c_tile)
        assert len(set(l_seg.flatten().tolist())) == 4 and int(c_seg.sum()) > 0
    # uncovered depths (den 0) read as label 0 in both
    part = cover.clone(); part[30:] = 0
    l_seg, c_seg = hip.seg_label_volume(a_seg, part.to(DEV), ptrs)
    l_tile, c_tile = tp.tile_label_volume(a_tile, (torch.ones(H, device=DEV), torch.ones(W, device=DEV), part.float().to(DEV)), ptrs)
    assert torch.equal(l_seg, l_tile) and torch.equal(c_seg, c_tile) and int(l_tile[..., 30:].sum()) == 0
    torch.cuda.synchronize()


def separated_logits(shape, C, g):
    """(*shape, C): |logit| <= 6, the channels of a voxel at least 0.02 apart, no logit within 1e-3 of 0: fp32 sigmoid keeps their order and side"""
    base = 9 * torch.rand(*shape, generator=g) - 4.5
    gaps = 0.02 + 0.4 * torch.rand(*shape, C, generator=g)
    steps = gaps.cumsum(-1) - gaps[..., :1]
    perm = torch.rand(*shape, C, generator=g).argsort(-1)
    l = (base.unsqueeze(-1) + steps.gather(-1, perm)).float()
    l = torch.where(l.abs() < 1e-3, torch.full_like(l, 1e-3), l)
    s = l.sort(-1).values
    assert float(l.abs().max()) <= 6 and float(l.abs().min()) >= 1e-3 and float((s[..., 1:] - s[..., :-1]).min()) >= 0.01
    return l


def test_one_tile_one_view_is_exact(mrdis):
    """one tile at an odd origin, one (w- and d-mirrored) view, Gaussian weights: pbar = fl(w p) / w keeps the side of 0.5 and the order of
    well-separated probabilities, an exact 0.5 stays 0.5 (w p is exact) and equal logits stay tied"""
    c = T.make_case('main', '')
    B, C, (TH, TW, TD), (H, W, D) = c['B'], c['C'], c['tile'], c['shape']
    origin, flips = (3, 2, 21), T.FLIP_W | T.FLIP_D
    g = torch.Generator().manual_seed(5)
    l = separated_logits((B, TH, TW, TD), C, g)                                                   # in VOLUME orientation
    l[0, 0, 0, 0] = torch.tensor([2.0, 2.0, 1.0]); l[0, 0, 1, 1] = torch.tensor([-1.0, 1.5, 1.5]); l[1, 5, 7, 15] = torch.tensor([0.75, 0.75, 0.75])
    l[0, 2, 3, 4] = torch.tensor([0.0, 0.0, 0.0]); l[1, 1, 1, 7] = torch.tensor([-2.0, 0.0, -1.0]); l[1, 3, 2, 9] = torch.tensor([0.0, 3.0, 0.0])
    c['geom'], c['logits'] = [(origin, flips)], [l.flip([2, 3]).contiguous()]                     # what the net gives for the mirrored input
    c['norms'] = [T.axis_norm(n, t, [o], w) for n, t, o, w in zip(c['shape'], c['tile'], origin, c['w'])]
    acc, labels, counts = run_kernels(mrdis, c)
    sl = (slice(None), slice(3, 3 + TH), slice(2, 2 + TW), slice(21, 21 + TD))
    mx = l.max(-1).values
    arg = torch.from_numpy(np.argmax(l.numpy(), axis=-1))
    want = torch.zeros(B, H, W, D, dtype=torch.int64)
    want[sl] = torch.where(mx > 0, arg + 1, torch.zeros_like(arg))
    assert torch.equal(labels.long(), want)
    assert labels[0, 3, 2, 21] == 1 and labels[0, 3, 3, 22] == 2 and labels[1, 8, 9, 36] == 1
    assert labels[0, 5, 5, 25] == 0 and labels[1, 4, 3, 28] == 0 and labels[1, 6, 4, 30] == 2
    # counts: mrdis_seg_counts of the tile + the labelled voxels outside it
    tw = c['tvol'][sl]
    region = torch.stack([(tw == k + 1).float() for k in range(C)], dim=-1)
    ref = mrdis.hip.seg_counts(l.to(DEV).permute(0, 4, 1, 2, 3), region.to(DEV).permute(0, 4, 1, 2, 3), logits=True).cpu()
    inside = torch.zeros(B, H, W, D, dtype=torch.bool); inside[sl] = True
    for k in range(C):
        ref[:, k, 2] += ((c['tvol'] == k + 1) & ~inside).flatten(1).sum(1).int()
    assert torch.equal(counts, ref)
    assert float(acc[~inside].abs().max()) == 0.0


def test_launch_counters_and_bit_identical_runs(mrdis):
    hip = mrdis.hip
    c = T.make_case('main', 'wd')
    before = hip.launch_counts()
    a1 = run_kernels(mrdis, c)
    mid = hip.launch_counts()
    assert mid['tileaccum'] - before['tileaccum'] == 2 * 2 * 4 * 4 == len(c['geom'])              # tiles x views
    assert mid['tilelabels'] - before['tilelabels'] == 1                                          # one per batch
    assert mid['segaccum'] == before['segaccum'] and mid['seglabels'] == before['seglabels']
    a2 = run_kernels(mrdis, c)
    for x, y in zip(a1, a2):
        assert torch.equal(x, y)
    # and the reverse: the sliding-window kernels do not count as tiles
    acc = torch.zeros(2, 9, 10, 37, 3, device=DEV)
    mid = hip.launch_counts()
    hip.seg_accum(torch.zeros(2, 9, 10, 16, 3, device=DEV).permute(0, 4, 1, 2, 3), acc, 0)
    hip.seg_label_volume(acc, torch.ones(37, dtype=torch.int32, device=DEV))
    after = hip.launch_counts()
    assert after['segaccum'] - mid['segaccum'] == 1 and after['seglabels'] - mid['seglabels'] == 1
    assert after['tileaccum'] == mid['tileaccum'] and after['tilelabels'] == mid['tilelabels']


def test_layouts_origins_and_alignment_are_refused(mrdis):
    hip, tp = mrdis.hip, mrdis.tilepred
    B, C, H, W, D, TH, TW, TD = 2, 3, 9, 10, 37, 6, 8, 16
    acc = torch.zeros(B, H, W, D, C, device=DEV)
    good = torch.zeros(B, TH, TW, TD, C, device=DEV).permute(0, 4, 1, 2, 3)
    w = tuple(torch.ones(n, device=DEV) for n in (TH, TW, TD))
    tp.tile_accum(good, acc, w, (H - TH, W - TW, D - TD), 13)
    bad = [
        (good, acc, w, (H - TH + 1, 0, 0), 0), (good, acc, w, (0, W - TW + 1, 0), 0), (good, acc, w, (0, 0, D - TD + 1), 0), (good, acc, w, (0, -1, 0), 0),
        (good, acc, w, (0, 0, 0), 2), (good, acc, w, (0, 0, 0), 32),                                                     # flip bits other than 1 | 4 | 8
        (torch.zeros(B, C, TH, TW, TD, device=DEV), acc, w, (0, 0, 0), 0),                                              # contiguous NCDHW
        (torch.zeros(B, TH, TW, 2 * TD, C, device=DEV)[:, :, :, ::2].permute(0, 4, 1, 2, 3), acc, w, (0, 0, 0), 0),    # holes
        (good, torch.zeros(B, H, W, D, 2 * C, device=DEV)[..., :C], w, (0, 0, 0), 0),                                   # acc not dense
        (good, torch.zeros(B, H, W, D, C + 1, device=DEV), w, (0, 0, 0), 0),                                            # channel counts differ
        (good, torch.zeros(B, H, W, TD - 1, C, device=DEV), w, (0, 0, 0), 0),                                           # tile deeper than the volume
        (good, acc.double(), w, (0, 0, 0), 0), (good.double(), acc, w, (0, 0, 0), 0),
        (good, acc.cpu(), w, (0, 0, 0), 0), (good, acc, (w[0], w[1], w[2].cpu()), (0, 0, 0), 0),                        # devices
        (good, acc, (w[0], w[1], w[2].double()), (0, 0, 0), 0), (good, acc, (w[0], w[1], torch.ones(TD + 1, device=DEV)), (0, 0, 0), 0),
        (good, torch.zeros(B * H * W * D * C + 1, device=DEV)[1:].view(B, H, W, D, C), w, (0, 0, 0), 0),                # acc 4-byte, not 16-byte aligned
    ]
    for call in bad:
        with pytest.raises(hip.MrdisError):
            tp.tile_accum(*call)
    c5 = torch.zeros(B, TH, TW, TD, 5, device=DEV).permute(0, 4, 1, 2, 3)
    with pytest.raises(hip.MrdisError):
        tp.tile_accum(c5, torch.zeros(B, H, W, D, 5, device=DEV), w, (0, 0, 0), 0)                # C = 5: the entry point's own refusal
    norms = tuple(torch.ones(n, device=DEV) for n in (H, W, D))
    for call in ((acc.permute(0, 2, 1, 3, 4), norms), (acc, (norms[0], norms[1], norms[2].long())), (acc, (norms[0], norms[1], torch.ones(2 * D, device=DEV)[::2])),
                 (acc, (norms[0].cpu(), norms[1], norms[2])), (acc, norms, torch.zeros(B + 1, dtype=torch.int64, device=DEV)),
                 (torch.zeros(B * H * W * D * C + 1, device=DEV)[1:].view(B, H, W, D, C), norms),
                 (torch.zeros(B, H, W, D, 5, device=DEV), norms)):
        with pytest.raises(hip.MrdisError):
            tp.tile_label_volume(*call)
    assert float(acc.sum()) == B * TH * TW * TD * C * 0.5                                         # only the one good call added (sigmoid(0) = 0.5)


# ----------------------------------------------------------------------------------------------- predict_tiles, VolumeLoader3D.tile and Run3D
CONTRASTS = ['T1', 'T1c', 'T2', 'T2_FLAIR']
SHAPE = (32, 48, 40)
TILE, STRIDE, MIRROR = (16, 32, 32), (8, 16, 8), 'hd'


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    """(store arrays, data_path with the three list files, the served test subjects): 32 x 48 x 40 volumes; the reader serves all but the first line of
    a list, so the test list's four subjects give three served ones: a batch of two and a batch of one"""
    data = data3d_volumes(n_subj=10, H=SHAPE[0], W=SHAPE[1], D=SHAPE[2], contrasts=CONTRASTS, seed=9)
    subj = data3d_subjects(data)
    root = tmp_path_factory.mktemp('tilepred')
    for name, part in (('train', subj[:3]), ('val', subj[3:6]), ('test', subj[6:10])):
        (root / f'fold_BraTS_3d_0_{name}_noval.txt').write_text('\n'.join(part) + '\n')
    return data, str(root), subj[7:10]


def _data(mrdis, world):
    store = mrdis.VolumeStore3D.from_arrays(world[0], DEV)
    return mrdis.VolumeData3D('BraTS', world[1], norm_type='z-score', batch_size=2, fold=0, shuffle=True, contrast_list=CONTRASTS, aug=True,
                              dropoff=True, store=store, device=DEV, region_channels=3, patch_size=TILE, patch_fg=0.0)


def _model(mrdis, seed=3):
    torch.manual_seed(seed)
    return mrdis.NVNet3D(TILE, 4, 3, 8, p=0.2).to(DEV)


def _collect(gen):
    res = {'subj_id': [], 'labels': [], 'counts': [], 'acc': []}
    for r in gen:
        res['subj_id'] += r['subj_id']
        res['tiles'], res['views'] = r['tiles'], r['views']
        for k in ('labels', 'counts', 'acc'):
            res[k].append(r[k].cpu())
    return {k: (torch.cat(v) if k in ('labels', 'counts', 'acc') else v) for k, v in res.items()}


@pytest.fixture(scope='module')
def predicted(mrdis, world):
    data, model = _data(mrdis, world), _model(mrdis)
    before = mrdis.hip.launch_counts()
    rng = torch.get_rng_state()
    res = _collect(mrdis.predict_tiles(model, data.testLoader, TILE, stride=STRIDE, mirror=MIRROR))
    assert torch.equal(torch.get_rng_state(), rng)                                               # no random stream is touched
    after = mrdis.hip.launch_counts()
    return data, model, res, {k: after[k] - before[k] for k in ('tileaccum', 'tilelabels', 'segaccum', 'seglabels', 'patchgather', 'volgather')}


def test_predict_tiles_equals_the_float64_composition(mrdis, world, predicted):
    data, model, res, launches = predicted
    loader = data.testLoader
    offs = mrdis.tile_offsets(SHAPE, TILE, STRIDE)
    assert offs == ([0, 8, 16], [0, 16], [0, 8]) and res['views'] == [0, T.FLIP_H, T.FLIP_D, T.FLIP_H | T.FLIP_D]
    assert res['tiles'] == [(h, w, d) for h in offs[0] for w in offs[1] for d in offs[2]]
    assert res['subj_id'] == world[2] and launches == {'tileaccum': 2 * 12 * 4, 'tilelabels': 2, 'segaccum': 0, 'seglabels': 0,
                                                       'patchgather': 2 * 12 * 4, 'volgather': 0}      # two batches x 12 tiles x 4 views, inputs only
    assert res['labels'].dtype == torch.uint8 and tuple(res['labels'].shape) == (3, *SHAPE) and tuple(res['counts'].shape) == (3, 3, 3)
    assert model.training                                                                         # the mode the caller had is put back
    # the float64 composition of the same net's per-tile outputs
    w = [T.weights(t, 'gaussian') for t in TILE]
    acc64, den64, n_acc, row = [], None, None, 0
    model.unet.eval()
    with torch.no_grad():
        for k, _, metas in loader.plain_plan():
            geom = [(o, v) for o in res['tiles'] for v in res['views']]
            logits = [model.unet(loader.tile(k, metas, o, flips=v)['inputs'])[0].permute(0, 2, 3, 4, 1).contiguous().cpu() for o, v in geom]
            c = dict(B=len(metas), C=3, shape=SHAPE, tile=TILE, w=w)
            a, den64, n_acc = T.oracle_acc(c, geom, logits)
            acc64.append(a)
    model.train()
    acc64 = np.concatenate(acc64)
    assert int(n_acc.max()) == 2 * 2 * 2 * 4 and int(n_acc.min()) == 4
    tvol = torch.stack([torch.from_numpy(np.asarray(world[0][s + '/seg'], dtype=np.float32)) for s in res['subj_id']])
    want, pred, lab, excused = T.oracle_labels(acc64, den64, tvol, True, T.excuse_bound(n_acc.max()))
    err = float((np.abs(res['acc'].double().numpy() - acc64) / den64[None, ..., None]).max())
    print(f'\n[tilepred predict_tiles] excused voxels {int(excused.sum())} of {excused.size}, predicted share {float(pred.mean()):.3f}, '
          f'max |acc - float64| / den {err:.3e}')
    T.assert_labels_counts(res['labels'], res['counts'], want, pred, lab, excused, 'predict_tiles')
    assert set(res['labels'].flatten().tolist()) <= {0, 1, 2, 4}
    # the axis sums the generator uploads are the oracle's
    norms = [mrdis.tile_norm(n, t, o, wa, 4 if a == 2 else 1) for a, (n, t, o, wa) in enumerate(zip(SHAPE, TILE, offs, w))]
    den32 = (norms[0][:, None] * norms[1][None, :])[:, :, None] * norms[2][None, None, :]
    assert float((np.abs(den32.astype(np.float64) - den64) / den64).max()) < 1e-6


def test_loader_tile_serves_the_stored_voxels_mirrored(mrdis, world, predicted):
    data = predicted[0]
    loader = data.testLoader
    k, _, metas = next(loader.plain_plan())
    origin = (5, 9, 3)
    plain = loader.tile(k, metas, origin)
    assert set(plain) == {'inputs', 'subj_id', 'slice_idx', 'mask', 'mask_host', 'batch_index', 'origins', 'table'}
    assert tuple(plain['inputs'].shape) == (2, 4, *TILE) and plain['inputs'].is_contiguous(memory_format=torch.channels_last_3d)
    for i, (sid, *_r) in enumerate(metas):
        for m, cn in enumerate(CONTRASTS):
            v = world[0].get(sid + '/' + cn)
            want = np.zeros(TILE, np.float32) if v is None else v[5:21, 9:41, 3:35]
            assert np.array_equal(plain['inputs'][i, m].cpu().numpy(), want), (sid, cn)
        assert int(loader.target_ptrs(plain)[i]) == data.store.ptr(sid + '/seg')
    both = loader.tile(k, metas, origin, flips=T.FLIP_H | T.FLIP_D)
    assert torch.equal(both['inputs'], plain['inputs'].flip([2, 4]))
    assert torch.equal(loader.tile(k, metas, origin, flips=T.FLIP_W)['inputs'], plain['inputs'].flip([3]))
    assert torch.equal(loader.tile(k, metas, (0, 0, 4), tile=(32, 48, 32))['inputs'], loader.window(k, metas, 4)['inputs'])
    for bad in (dict(origin=(17, 0, 0)), dict(origin=(0, 0, 9)), dict(origin=(0, -1, 0)), dict(origin=(0, 0)), dict(origin=(0, 0, 0), flips=2),
                dict(origin=(0, 0, 0), flips=True), dict(origin=(0, 0, 0), tile=(16, 32, 48)), dict(origin=(0, 0, 0), tile=(16, 32))):
        with pytest.raises(ValueError):
            loader.tile(k, metas, **bad)
    with pytest.raises(ValueError):
        next(mrdis.predict_tiles(predicted[1], data.trainLoader, TILE))                           # aug
    with pytest.raises(ValueError):
        next(mrdis.predict_tiles(predicted[1], data.testLoader, (16, 32, 48)))                    # deeper than the volume


def test_whole_plane_uniform_h_mirror_is_predict_volumes_with_flip(mrdis, world, predicted):
    data, model = predicted[0], predicted[1]
    H, W, _ = SHAPE
    Dz = data.testLoader.dataset.crop()[1]
    assert Dz == 32
    tiles = _collect(mrdis.predict_tiles(model, data.testLoader, (H, W, Dz), weight='uniform', mirror='h'))
    assert tiles['tiles'] == [(0, 0, 0), (0, 0, 8)] and tiles['views'] == [0, T.FLIP_H]
    vols = {'subj_id': [], 'labels': [], 'counts': [], 'acc': []}
    for r in mrdis.predict_volumes(model, data.testLoader, flip=True):
        vols['subj_id'] += r['subj_id']
        for key in ('labels', 'counts', 'acc'):
            vols[key].append(r[key].cpu())
    assert tiles['subj_id'] == vols['subj_id'] == world[2]
    for key in ('acc', 'labels', 'counts'):
        assert torch.equal(tiles[key], torch.cat(vols[key])), key
    assert float(tiles['acc'].max()) > 0


RUN_CFG = dict(dataset_name='BraTS', contrast_list=CONTRASTS, batch_size=2, model_name='NVNet3D', init_channels=8, epochs=1, lr=1e-4, device='cuda:0',
               seed=10, patch_size=list(TILE), patch_fg=0.0, max_batches=1)


def test_run3d_with_predict_tile_writes_the_same_files(mrdis, world, tmp_path):
    hip = mrdis.hip
    cfg = dict(RUN_CFG, data_path=world[1], ckpt_path=str(tmp_path / 'ckpt'))
    store = mrdis.VolumeStore3D.from_arrays(world[0], DEV)
    mrdis.Run3D(cfg, store=store, log=lambda *a: None).train()
    pred = dict(cfg, phase='predict', max_batches=None, predict_regions=True, predict_post=True)
    out = os.path.join(cfg['ckpt_path'], 'result_test')

    def files():
        return sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)

    # predict_tile null: the depth window, and no tile kernel
    before = hip.launch_counts()
    stat0 = mrdis.Run3D(pred, store=store, log=lambda *a: None).predict()
    mid = hip.launch_counts()
    assert mid['tileaccum'] == before['tileaccum'] and mid['tilelabels'] == before['tilelabels']
    assert mid['segaccum'] - before['segaccum'] == 2 * 2 and mid['seglabels'] - before['seglabels'] == 2
    plain_files = files()
    assert [f for f in plain_files if f.endswith('_seg.npy') and os.sep not in f] == [f'{s}_seg.npy' for s in world[2]]
    os.rename(out, out + '_window')
    # predict_tile set: the tiles, and no window kernel; the same set of files
    stat1 = mrdis.Run3D(dict(pred, predict_tile=list(TILE), predict_mirror='h'), store=store, log=lambda *a: None).predict()
    after = hip.launch_counts()
    assert after['tileaccum'] - mid['tileaccum'] == 2 * (3 * 2 * 2) * 2 and after['tilelabels'] - mid['tilelabels'] == 2      # batches x tiles x views
    assert after['segaccum'] == mid['segaccum'] and after['seglabels'] == mid['seglabels']
    assert files() == plain_files and set(stat1) == set(stat0) and stat1['n'] == 3
    for s in world[2]:
        for sub in ('', 'post'):
            v = np.load(os.path.join(out, sub, f'{s}_seg.npy'))
            assert v.dtype == np.uint8 and v.shape == SHAPE and set(np.unique(v).tolist()) <= {0, 1, 2, 4}
    rows = open(os.path.join(out, 'predict.csv')).read().splitlines()
    assert rows[0] == 'subj_id,dice,iou' and [r.split(',')[0] for r in rows[1:]] == world[2]
    # a tile that does not fit the volumes, or that the net does not accept, is refused by name before anything runs
    with pytest.raises(ValueError, match='predict_tile'):
        mrdis.Run3D(dict(pred, predict_tile=[16, 32, 48]), store=store, log=lambda *a: None)
    with pytest.raises(ValueError, match='predict_tile'):
        mrdis.Run3D(dict(pred, predict_tile=[16, 32, 20]), store=store, log=lambda *a: None)
    assert hip.launch_counts()['tileaccum'] == after['tileaccum']
