"""Connected components and label clean-up on the GPU: the kernels of csrc/mrdis_cc.hip (hip.cc_label / mrdis.components3d, hip.cc_clean /
mrdis.clean_labels) and `Run3D` with predict_post / phase=postprocess / score_subdir.

Everything is integers, so every comparison is for equality.  The oracles are the numpy labeller and the plain-Python rules of
tests/postproc_check.py (checked on the CPU by tests/test_postproc_cpu.py).  The labelling kernels tile a sample into 4 x 4 x 64 voxels
(H x W x D); which shape takes which path:
  (1,1,1,1) (1,1,1,64) (1,4,4,64)   one tile, partly / wholly filled: the LDS union-find alone, the merge finds nothing to do
  (1,5,7,9) (1,3,5,65)              one voxel beyond a tile in H / W / D: tiles that hold a single plane, row or column
  (1,3,3,63)                        one voxel short of a tile in every axis
  (2,33,17,70) (1,9,5,129)          several tiles along every axis, the last ones cut; two samples
  (1,2,3,257) (1,257,2,3) (1,3,257,2)   one long axis: 5 tiles along D / 65 along H / 65 along W
Densities 0.2 / 0.35 / 0.5 bracket the site-percolation threshold of the cubic lattice (0.31 at c = 6): long tortuous clusters across tiles."""
import os
import shutil

import numpy as np
import pytest
import torch

from fixtures_data3d import data3d_volumes, data3d_subjects
from postproc_check import np_clean, np_components_batch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
CONN = (6, 18, 26)
FG = (1, 2, 4)
TH, TW, TD = 4, 4, 64                                                # the tile of csrc/mrdis_cc.hip
SHAPES = [(1, 1, 1, 1), (1, 1, 1, 64), (1, 5, 7, 9), (2, 33, 17, 70), (1, 2, 3, 257), (1, 257, 2, 3), (1, 3, 257, 2),
          (1, 4, 4, 64), (1, 3, 5, 65), (1, 3, 3, 63), (1, 9, 5, 129)]


@pytest.fixture(scope='module')
def mrdis():
    import mrdis as m
    return m


def run_label(mrdis, labels, c, fg=FG):
    comp, size = mrdis.components3d(torch.from_numpy(np.ascontiguousarray(labels)).to(DEV), fg=fg, connectivity=c)
    assert comp.dtype == torch.int32 and size.dtype == torch.int32 and tuple(comp.shape) == tuple(labels.shape) == tuple(size.shape)
    return comp.cpu().numpy(), size.cpu().numpy()


def assert_labelling(mrdis, labels, c, fg=FG):
    """kernels == oracle, plus the properties that need no oracle"""
    comp, size = run_label(mrdis, labels, c, fg)
    want_comp, want_size = np_components_batch(labels, fg, c)
    assert np.array_equal(comp, want_comp), f'comp differs at {int((comp != want_comp).sum())} voxels'
    assert np.array_equal(size, want_size), f'size differs at {int((size != want_size).sum())} voxels'
    B = labels.shape[0]
    idx = np.arange(labels[0].size, dtype=np.int64).reshape(labels.shape[1:])
    for b in range(B):
        fgv = np.isin(labels[b], fg)
        assert int(size[b].sum()) == int(fgv.sum())
        assert np.array_equal(size[b] > 0, comp[b] == idx) and np.array_equal(comp[b] >= 0, fgv)
    return comp, size


def random_labels(shape, density, seed):
    rng = np.random.RandomState(seed)
    fg = rng.rand(*shape) < density
    return np.where(fg, rng.choice(np.array(FG, np.uint8), size=shape), 0).astype(np.uint8)


# ----------------------------------------------------------------------------------------------- shapes against tiling
@pytest.mark.parametrize('c', CONN)
@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_random_volumes_equal_the_oracle(mrdis, shape, c):
    for i, density in enumerate((0.2, 0.35, 0.5)):
        assert_labelling(mrdis, random_labels(shape, density, seed=7 * i + c), c)
    full = np.full(shape, 2, np.uint8)
    comp, size = assert_labelling(mrdis, full, c)
    P = shape[1] * shape[2] * shape[3]
    assert (comp == 0).all() and (size[:, 0, 0, 0] == P).all() and int(size.sum()) == shape[0] * P          # one component per sample
    comp, size = assert_labelling(mrdis, np.zeros(shape, np.uint8), c)
    assert (comp == -1).all() and not size.any()
    cleaned, stats = mrdis.clean_labels(torch.zeros(shape, dtype=torch.uint8, device=DEV), connectivity=c, min_voxels=3, keep='largest',
                                        et_min_voxels=5)
    assert not cleaned.any() and tuple(stats.shape) == (shape[0], 6) and stats.dtype == torch.int32 and not stats.any()


# ----------------------------------------------------------------------------------------------- structures that break labellers
SH = (9, 11, 130)                                                    # 3 x 3 x 3 tiles, the last of each axis cut


def serpentine(H, W, D):
    """one chain through the whole volume: every other D line of every other plane, joined to the next at alternating ends"""
    m = np.zeros((H, W, D), np.uint8)
    end = D - 1
    ws = list(range(0, W, 2))
    for hi, h in enumerate(range(0, H, 2)):
        order = ws if hi % 2 == 0 else ws[::-1]
        for j, w in enumerate(order):
            m[h, w, :] = 1
            if j + 1 < len(order):
                m[h, (w + order[j + 1]) // 2, end] = 1
                end = D - 1 - end
        if h + 2 < H:
            m[h + 1, order[-1], end] = 1
            end = D - 1 - end
    return m


def structures():
    H, W, D = SH
    out = {}
    out['serpentine'] = serpentine(H, W, D)[None]
    comb = np.zeros(SH, np.uint8); comb[::2, ::2, :] = 1; comb[:, :, D - 1] = 1        # arms along D that only join in the last d plane
    u = np.zeros(SH, np.uint8); u[:, ::2, ::2] = 2; u[H - 1, :, :] = 2                  # arms along H that only join in the last h plane
    out['comb'] = np.stack([comb, u])
    h, w, d = np.meshgrid(np.arange(H), np.arange(W), np.arange(D), indexing='ij')
    out['checkerboard'] = (((h + w + d) % 2 == 0) * 4).astype(np.uint8)[None]
    pairs = np.zeros((4,) + SH, np.uint8)
    pairs[0, 1, 1, 10] = pairs[0, 2, 2, 10] = 1                      # touch by an edge, inside a tile
    pairs[1, 3, 3, 70] = pairs[1, 4, 4, 70] = 1                      # by an edge, across a tile edge
    pairs[2, 1, 1, 10] = pairs[2, 2, 2, 11] = 1                      # by a corner, inside a tile
    pairs[3, 3, 3, 63] = pairs[3, 4, 4, 64] = 1                      # by a corner, across a tile corner
    pairs[3, 7, 8, 63] = pairs[3, 8, 7, 64] = 2                      # the same with an offset of mixed signs (+h, -w, +d)
    out['pairs'] = pairs
    nowrap = np.zeros((3,) + SH, np.uint8)
    nowrap[0, 2, 3, D - 1] = nowrap[0, 2, 4, 0] = 1                  # the end of a D line and the start of the next
    nowrap[0, 5, W - 1, 40] = nowrap[0, 6, 0, 40] = 1                # the end of a W row and the start of the next plane
    nowrap[0, H - 1, W - 1, D - 1] = nowrap[1, 0, 0, 0] = 1          # the last voxel of a sample and the first of the next
    nowrap[1, H - 1, W - 1, D - 1] = nowrap[2, 0, 0, 0] = 1
    nowrap[2, 4, W - 1, D - 1] = nowrap[2, 5, 0, 0] = 1              # the end of a plane's last line and the start of the next plane
    out['nowrap'] = nowrap
    cross = np.zeros(SH, np.uint8)                                   # three lines through a tile corner: every face is crossed, in both directions
    cross[1:8, 4, 64] = 1; cross[4, 1:10, 64] = 2; cross[4, 4, 3:128] = 4
    diag = np.zeros(SH, np.uint8)
    for k in range(9):
        diag[k, k, 60 + k] = 1                                       # a corner-connected diagonal through the tile corners (4, 4, 64) and (8, 8, 64 ..)
    out['cross'] = np.stack([cross, diag])
    bridge = np.zeros(SH, np.uint8)
    bridge[4, 4, 60:67] = [1, 8, 1, 255, 1, 3, 1]                    # 8, 255 and a label outside fg between foreground voxels: no bridge
    bridge[3:6, 7, 64] = [2, 7, 2]
    out['bridge'] = bridge[None]
    return out


STRUCTURES = structures()


@pytest.mark.parametrize('c', CONN)
@pytest.mark.parametrize('name', list(STRUCTURES))
def test_structures_equal_the_oracle(mrdis, name, c):
    labels = STRUCTURES[name]
    comp, size = assert_labelling(mrdis, labels, c)
    ncomp = [int((s > 0).sum()) for s in size]
    if name == 'serpentine':
        assert ncomp == [1] and int(size[0, 0, 0, 0]) == int((labels > 0).sum())
    elif name == 'comb':
        assert ncomp == [1, 1] and (comp[labels > 0] == 0).all()
    elif name == 'checkerboard':
        assert ncomp == ([int((labels > 0).sum())] if c == 6 else [1])                 # c = 6: singletons only
    elif name == 'pairs':
        assert ncomp == {6: [2, 2, 2, 4], 18: [1, 1, 2, 4], 26: [1, 1, 1, 2]}[c]
    elif name == 'nowrap':
        assert ncomp == [5, 2, 3] and int(size.max()) == 1                              # every voxel stays on its own
    elif name == 'cross':
        assert ncomp == [1, 1 if c == 26 else 9]
    elif name == 'bridge':
        assert ncomp == [6] and int(size.max()) == 1
        t = torch.from_numpy(labels).to(DEV)
        cleaned, stats = mrdis.clean_labels(t, connectivity=c, min_voxels=2)            # the singletons go, 8 / 255 / 3 / 7 pass through unchanged
        want, want_stats = np_clean(labels, FG, c, min_voxels=2)
        assert np.array_equal(cleaned.cpu().numpy(), want) and np.array_equal(stats.cpu().numpy(), want_stats)
        assert sorted(np.unique(want).tolist()) == [0, 3, 7, 8, 255] and stats.cpu().tolist() == [[6, 0, 6, 6, 0, 0]]


# ----------------------------------------------------------------------------------------------- properties
def test_runs_repeat_and_input_forms_agree(mrdis):
    labels = random_labels((2, 33, 17, 70), 0.33, seed=3)
    t = torch.from_numpy(labels).to(DEV)
    a = mrdis.components3d(t, connectivity=6)
    b = mrdis.components3d(t, connectivity=6)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])                          # identical bits
    c3 = mrdis.components3d(t[1], connectivity=6)                                        # a 3-D input = the B = 1 4-D one
    c4 = mrdis.components3d(t[1:2], connectivity=6)
    assert c3[0].dim() == 3 and torch.equal(c3[0], c4[0][0]) and torch.equal(c3[1], c4[1][0]) and torch.equal(c3[0], a[0][1])
    # a non-contiguous view is handled as edt3d_sq handles one: the result is that of its contiguous copy, in the view's own index order
    big = torch.from_numpy(random_labels((2, 17, 33, 70), 0.33, seed=4)).to(DEV)
    view = big.permute(0, 2, 1, 3)
    assert not view.is_contiguous()
    got = mrdis.components3d(view, connectivity=18)
    want = mrdis.components3d(view.contiguous(), connectivity=18)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert np.array_equal(got[0].cpu().numpy(), np_components_batch(view.cpu().numpy(), FG, 18)[0])
    cl = mrdis.clean_labels(view[:, :, ::2], min_voxels=3)
    cw = np_clean(view[:, :, ::2].cpu().numpy(), FG, 26, min_voxels=3)
    assert np.array_equal(cl[0].cpu().numpy(), cw[0]) and np.array_equal(cl[1].cpu().numpy(), cw[1])
    # a bool / uint8 mask with fg = (1,)
    mask = t > 0
    mb = mrdis.components3d(mask, fg=(1,), connectivity=26)
    mu = mrdis.components3d(mask.to(torch.uint8), fg=(1,), connectivity=26)
    full = mrdis.components3d(t, connectivity=26)
    assert torch.equal(mb[0], mu[0]) and torch.equal(mb[0], full[0]) and torch.equal(mb[1], full[1])
    cleaned, stats = mrdis.clean_labels(t[0], min_voxels=2)                              # a 3-D input: a 3-D volume, stats (1, 6)
    assert cleaned.dim() == 3 and tuple(stats.shape) == (1, 6)


# ----------------------------------------------------------------------------------------------- clean_labels against np_clean
def clean_volume():
    """(3, 20, 18, 70) labels {0, 1, 2, 4}.  Sample 0: two blobs of 60 voxels (the tie for largest; the second holds ET), a blob of 45 with
    ET, specks of 1 .. 3 voxels, some of them ET.  Sample 1: no foreground.  Sample 2: a blob of oedema and ET specks of at most 3 voxels:
    its ET lies only in components that min_voxels = 4 removes."""
    v = np.zeros((3, 20, 18, 70), np.uint8)
    v[0, 2:5, 2:6, 3:8] = 2                                          # 3 x 4 x 5 = 60
    v[0, 10:13, 10:14, 60:65] = 1; v[0, 11, 11:13, 61:64] = 4        # 60 again, across the tile face d = 64, six of them ET
    v[0, 15:18, 2:5, 30:35] = 2; v[0, 16, 3, 31:34] = 4              # 45, three of them ET
    v[0, 0, 17, 69] = 4; v[0, 8, 0, 0:2] = 4; v[0, 19, 9, 40:43] = 1; v[0, 7, 8, 20] = 2; v[0, 6, 9, 21] = 2      # specks (the last two touch by a corner)
    v[2, 5:9, 5:9, 10:20] = 2
    v[2, 0, 0, 0] = 4; v[2, 15, 15, 63:65] = 4; v[2, 19, 17, 67:70] = 4
    return v


@pytest.fixture(scope='module')
def clean_case(mrdis):
    v = clean_volume()
    return v, torch.from_numpy(v).to(DEV)


@pytest.mark.parametrize('c', (6, 26))
@pytest.mark.parametrize('keep', ('all', 'largest'))
def test_clean_labels_equal_the_rules(mrdis, clean_case, keep, c):
    v, t = clean_case
    assert sorted(np.unique(v).tolist()) == [0, 1, 2, 4] and not v[1].any()
    for min_voxels in (0, 1, 4, 10 ** 6):
        _, base = np_clean(v, FG, c, min_voxels=min_voxels, keep=keep)
        ns = sorted({int(n) for n in base[:, 4]} | {int(n) + 1 for n in base[:, 4]} | {0})      # 0, n and n + 1 for every sample's actual n
        for et_min in ns:
            want, want_stats = np_clean(v, FG, c, min_voxels=min_voxels, keep=keep, et_min_voxels=et_min)
            got, stats = mrdis.clean_labels(t, connectivity=c, min_voxels=min_voxels, keep=keep, et_min_voxels=et_min)
            what = (keep, c, min_voxels, et_min)
            assert np.array_equal(stats.cpu().numpy(), want_stats), (what, stats.cpu().tolist(), want_stats.tolist())
            assert np.array_equal(got.cpu().numpy(), want), what
            again, stats2 = mrdis.clean_labels(got, connectivity=c, min_voxels=min_voxels, keep=keep, et_min_voxels=et_min)
            assert torch.equal(again, got), what                      # clean(clean(x)) == clean(x)
            assert int(stats2[:, 3].sum()) == 0


def test_clean_cases_cover_the_ties_and_defaults(mrdis, clean_case):
    v, t = clean_case
    got, stats = mrdis.clean_labels(t)                               # the defaults: byte for byte the input
    assert torch.equal(got, t) and got.data_ptr() != t.data_ptr()
    st = stats.cpu().numpy()
    assert st[:, 3].tolist() == [0, 0, 0] and st[:, 5].tolist() == [0, 0, 0] and st[1].tolist() == [0] * 6
    assert np.array_equal(st, np_clean(v)[1]) and np.array_equal(st[:, 0], st[:, 1])
    _, size = mrdis.components3d(t)
    sizes = np.sort(size[0].cpu().numpy().reshape(-1))[::-1]
    assert sizes[0] == sizes[1] == 60 and sizes[2] == 45              # the tie for largest
    got, stats = mrdis.clean_labels(t, keep='largest')
    g = got.cpu().numpy()
    assert (g[0, 2:5, 2:6, 3:8] == 2).all() and int((g[0] > 0).sum()) == 60 and not g[1].any()      # the tie goes to the smaller root
    assert stats.cpu()[:, 1].tolist() == [1, 0, 1]
    got, stats = mrdis.clean_labels(t, min_voxels=4, et_min_voxels=1000)
    st = stats.cpu().numpy()
    assert st[2].tolist() == [4, 1, 166, 6, 0, 0]                    # sample 2: its ET went with the removed components, nothing to replace
    assert st[0, 4] == 9 and st[0, 5] == 1 and not (got[0] == 4).any() and int((got[0] == 1).sum()) == 54 + 9
    # other labels: et_label = 2 -> 7 in a sample whose oedema is below the threshold
    got, stats = mrdis.clean_labels(t, fg=(1, 2, 4, 7), et_label=2, et_min_voxels=10 ** 6, et_replace=7)
    want, want_stats = np_clean(v, (1, 2, 4, 7), 26, et_label=2, et_min_voxels=10 ** 6, et_replace=7)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(stats.cpu().numpy(), want_stats) and (want == 7).any()


# ----------------------------------------------------------------------------------------------- launch counters
def counts_delta(hip, fn):
    before = hip.launch_counts(elem=True)
    fn()
    after = hip.launch_counts(elem=True)
    return {k: after[k] - before[k] for k in before if after[k] != before[k]}


def test_launch_counts_are_fixed(mrdis):
    hip = mrdis.hip
    cases = [np.zeros((1, 1, 1, 1), np.uint8), np.ones((1, 1, 1, 1), np.uint8), np.zeros((2, 33, 17, 70), np.uint8), np.full((2, 33, 17, 70), 4, np.uint8),
             random_labels((3, 33, 17, 70), 0.3, 1), random_labels((1, 33, 17, 70), 0.3, 2), STRUCTURES['serpentine']]
    seen = set()
    for labels in cases:
        t = torch.from_numpy(labels).to(DEV)
        for c in CONN:
            d = counts_delta(hip, lambda: mrdis.components3d(t, connectivity=c))
            assert set(d) == {'cclabel', 'all'} and d['all'] == d['cclabel'], d          # no other family moves
            seen.add(d['cclabel'])
        d = counts_delta(hip, lambda: mrdis.clean_labels(t, min_voxels=2, keep='largest', et_min_voxels=3))
        assert set(d) == {'cclabel', 'ccclean', 'all'} and d['ccclean'] == 1, d
        seen.add(d['cclabel'])
        comp, size = hip.cc_label(t, 0b10110, 26)
        d = counts_delta(hip, lambda: hip.cc_clean(t, comp, size, 2, True, 4, 3, 1))
        assert set(d) == {'ccclean', 'all'} and d['ccclean'] == 1 and d['all'] == 4, d
    assert seen == {hip.CC_LABEL_LAUNCHES} == {3}                                        # the same constant for every B, shape and content


# ----------------------------------------------------------------------------------------------- closing the loop with scoring
def test_cleaning_repairs_the_region_scores(mrdis):
    shape = (1, 24, 20, 70)
    truth = np.zeros(shape, np.uint8)
    truth[0, 3:6, 3:6, 5:10] = 2; truth[0, 4, 4, 5:10] = 1           # 45 voxels, 42 of them on the surface
    pred = truth.copy()
    pred[0, 23, 19, 67:70] = 2                                       # a three-voxel speck in the opposite corner: 3 of 45 surface voxels, beyond the 95 % rank
    t, p = torch.from_numpy(truth).to(DEV), torch.from_numpy(pred).to(DEV)
    before = mrdis.region_scores(p, t)
    assert float(before['hd95'][0, 0]) > 0 and float(before['dice'][0, 0]) < 1
    cleaned, stats = mrdis.clean_labels(p, min_voxels=4)
    after = mrdis.region_scores(cleaned, t)
    assert float(after['hd95'][0, 0]) == 0.0 and float(after['dice'][0, 0]) == 1.0 and torch.equal(cleaned, t)
    assert stats.cpu().tolist() == [[2, 1, int((pred > 0).sum()), 3, 0, 0]]
    # five ET voxels in a subject whose ground truth has none (inside the tumour core, so that WT and TC are untouched)
    pred = truth.copy()
    pred[0, 4, 4, 5:10] = 4
    p = torch.from_numpy(pred).to(DEV)
    before = mrdis.region_scores(p, t)
    assert float(before['dice'][0, 2]) == 0.0
    cleaned, stats = mrdis.clean_labels(p, et_min_voxels=6)
    after = mrdis.region_scores(cleaned, t)
    assert float(after['dice'][0, 2]) == 1.0 and float(after['hd95'][0, 2]) == 0.0 and torch.equal(cleaned, t)
    assert stats.cpu().tolist() == [[1, 1, int((pred > 0).sum()), 0, 5, 1]]
    assert torch.equal(mrdis.clean_labels(p, et_min_voxels=5)[0], p)                     # n = 5 is not below 5


# ----------------------------------------------------------------------------------------------- Run3D: predict_post, phase postprocess, score_subdir
CONTRASTS = ['T1', 'T1c', 'T2', 'T2_FLAIR']
RUN_CFG = dict(dataset_name='BraTS', contrast_list=CONTRASTS, batch_size=2, model_name='NVNet3D', init_channels=8, epochs=1, lr=1e-4,
               device='cuda:0', seed=10, predict_stride=16)
POST = dict(post_connectivity=6, post_min_voxels=30, post_keep='all', post_et_min_voxels=10 ** 6)
POST_FG = (1, 2, 3, 4, 5, 6, 7)
QUIET = dict(log=lambda *a: None)


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    """the tiny world of tests/test_gpu_segvol.py: 32 x 32 x 123 volumes, three served test subjects (a batch of two and a batch of one)"""
    data = data3d_volumes(n_subj=11, H=32, W=32, D=123, contrasts=CONTRASTS, seed=9)
    subj = data3d_subjects(data)
    root = tmp_path_factory.mktemp('postproc')
    for name, part in (('train', subj[:4]), ('val', subj[4:7]), ('test', subj[7:11])):
        (root / f'fold_BraTS_3d_0_{name}_noval.txt').write_text('\n'.join(part) + '\n')
    return data, str(root), subj[8:11]


@pytest.fixture(scope='module')
def predicted(mrdis, world, tmp_path_factory):
    """one epoch of training, then phase predict three times on the same checkpoint: plain, with predict_post and predict_regions, and with
    predict_regions alone; with the launch-count deltas of the first two"""
    cfg = dict(RUN_CFG, data_path=world[1], ckpt_path=str(tmp_path_factory.mktemp('ckpt')))
    store = mrdis.VolumeStore3D.from_arrays(world[0], DEV)
    mrdis.Run3D(cfg, store=store, **QUIET).train()
    dirs = {}
    for name in ('plain', 'post', 'regions'):
        dirs[name] = str(tmp_path_factory.mktemp(name) / 'ckpt')
        shutil.copytree(cfg['ckpt_path'], dirs[name])
    hip = mrdis.hip
    c0 = hip.launch_counts()
    plain = mrdis.Run3D(dict(cfg, phase='predict', ckpt_path=dirs['plain']), store=store, **QUIET).predict()
    c1 = hip.launch_counts()
    post = mrdis.Run3D(dict(cfg, phase='predict', ckpt_path=dirs['post'], predict_post=True, predict_regions=True, **POST), store=store, **QUIET).predict()
    c2 = hip.launch_counts()
    regions = mrdis.Run3D(dict(cfg, phase='predict', ckpt_path=dirs['regions'], predict_regions=True), store=store, **QUIET).predict()
    c3 = hip.launch_counts()
    return dict(cfg=cfg, store=store, dirs=dirs, plain=plain, post=post, regions=regions, off={k: c1[k] - c0[k] for k in c0},
                on={k: c2[k] - c1[k] for k in c0}, reg={k: c3[k] - c2[k] for k in c0})


def read_bytes(*parts):
    with open(os.path.join(*parts), 'rb') as f:
        return f.read()


def test_predict_post_off_launches_nothing_and_changes_nothing(mrdis, world, predicted):
    p = predicted
    assert all(p['off'][k] == 0 for k in mrdis.hip.CC_FAMILIES) and all(p['reg'][k] == 0 for k in mrdis.hip.CC_FAMILIES)
    out = os.path.join(p['dirs']['plain'], 'result_test')
    assert sorted(os.listdir(out)) == sorted([f'{s}_seg.npy' for s in world[2]] + ['predict.csv'])            # the files of today, no post/
    assert set(p['plain']) == {'dice', 'iou', 'n'} and p['plain']['n'] == 3
    assert sorted(os.listdir(os.path.join(p['dirs']['regions'], 'result_test'))) == \
        sorted([f'{s}_seg.npy' for s in world[2]] + ['predict.csv', 'predict_regions.csv'])


def test_predict_post_writes_cleaned_volumes_beside_unchanged_raw_files(mrdis, world, predicted):
    p = predicted
    hip = mrdis.hip
    on, reg = p['on'], p['reg']
    assert on['cclabel'] == 2 * hip.CC_LABEL_LAUNCHES and on['ccclean'] == 2                                    # two batches
    assert on['regsurf'] == 2 * reg['regsurf'] == 4                                                             # raw and cleaned labels are scored
    rest = hip.CC_FAMILIES + hip.SURFDIST_FAMILIES + ('all',)
    assert {k: v for k, v in on.items() if k not in rest} == {k: v for k, v in reg.items() if k not in rest}
    assert on['all'] - reg['all'] == 2 * (3 + 4 + 4)                                                            # labelling, rules, one more scoring
    raw, ref = os.path.join(p['dirs']['post'], 'result_test'), os.path.join(p['dirs']['regions'], 'result_test')
    names = [f'{s}_seg.npy' for s in world[2]]
    assert sorted(os.listdir(raw)) == sorted(names + ['predict.csv', 'predict_regions.csv', 'post'])
    for n in names + ['predict.csv', 'predict_regions.csv']:
        assert read_bytes(raw, n) == read_bytes(ref, n), n                                                      # the raw files are unchanged
    for n in names + ['predict.csv']:
        assert read_bytes(raw, n) == read_bytes(p['dirs']['plain'], 'result_test', n), n
    post = os.path.join(raw, 'post')
    assert sorted(os.listdir(post)) == sorted(names + ['postprocess.csv', 'predict_regions.csv'])
    vols = np.stack([np.load(os.path.join(raw, n)) for n in names])
    want, want_stats = np_clean(vols, POST_FG, 6, min_voxels=30, keep='all', et_label=4, et_min_voxels=10 ** 6, et_replace=1)
    assert int(want_stats[:, 3].sum()) > 0 or int(want_stats[:, 5].sum()) > 0                                   # the cleaning did something
    rows = open(os.path.join(post, 'postprocess.csv')).read().splitlines()
    assert rows[0] == 'subj_id,components,kept,foreground,removed,et_voxels,et_replaced'
    for i, (sid, n) in enumerate(zip(world[2], names)):
        got = np.load(os.path.join(post, n))
        assert got.dtype == np.uint8 and np.array_equal(got, want[i]), sid
        assert rows[1 + i] == sid + ',' + ','.join(str(int(x)) for x in want_stats[i]), sid
    assert len(rows) == 4
    # post/predict_regions.csv: the region scores of the cleaned labels
    regs = open(os.path.join(post, 'predict_regions.csv')).read().splitlines()
    assert regs[0] == mrdis.train3d.region_csv_header() and [r.split(',')[0] for r in regs[1:]] == world[2]
    for i, sid in enumerate(world[2]):
        seg = np.asarray(world[0][sid + '/seg'], dtype=np.float32)
        res = mrdis.region_scores(torch.from_numpy(want[i][None]).to(DEV), torch.from_numpy(seg[None]).to(DEV))
        wantrow = [float(res[k][0, r]) for k in ('dice', 'sensitivity', 'specificity', 'hd95') for r in range(3)]
        gotrow = [float(x) for x in regs[1 + i].split(',')[1:]]
        assert all(g == w or (g != g and w != w) for g, w in zip(gotrow, wantrow)), (sid, gotrow, wantrow)
    stat = p['post']
    assert stat['dice'] == p['plain']['dice'] and stat['iou'] == p['plain']['iou']
    for i, col in enumerate(mrdis.postproc.STATS_COLUMNS):
        assert stat[f'post_{col}'] == pytest.approx(float(want_stats[:, i].mean()), abs=1e-12)
    assert all(stat[k] == p['regions'][k] for k in p['regions'])


def test_phase_postprocess_and_score_subdir_reproduce_the_files(mrdis, world, predicted, tmp_path):
    p = predicted
    src = os.path.join(p['dirs']['post'], 'result_test')
    work = str(tmp_path / 'ckpt')
    os.makedirs(os.path.join(work, 'result_test'))
    names = [f'{s}_seg.npy' for s in world[2]]
    for n in names:                                                  # the raw files alone: no checkpoint, no csv
        shutil.copy(os.path.join(src, n), os.path.join(work, 'result_test', n))
    cfg = dict(p['cfg'], ckpt_path=work, **POST)
    before = mrdis.hip.launch_counts()
    run = mrdis.Run3D(dict(cfg, phase='postprocess'), store=p['store'], **QUIET)
    assert run.model is None and run.optimizer is None
    stat = run.postprocess()
    after = mrdis.hip.launch_counts()
    assert after['all'] - before['all'] == 2 * (3 + 4 + 4) and after['cclabel'] - before['cclabel'] == 6 and after['ccclean'] - before['ccclean'] == 2
    assert stat['n'] == 3 and stat['removed'] == p['post']['post_removed'] and stat['dice_wt'] == p['post']['post_dice_wt']
    post = os.path.join(work, 'result_test', 'post')
    files = names + ['postprocess.csv', 'predict_regions.csv']
    assert sorted(os.listdir(post)) == sorted(files) and sorted(os.listdir(os.path.join(work, 'result_test'))) == sorted(names + ['post'])
    for n in files:
        assert read_bytes(post, n) == read_bytes(src, 'post', n), n                     # byte for byte what predict wrote
    # phase score with score_subdir = post reproduces post/predict_regions.csv; with '' it reads and writes the raw directory
    want = read_bytes(post, 'predict_regions.csv')
    os.remove(os.path.join(post, 'predict_regions.csv'))
    mrdis.Run3D(dict(cfg, phase='score', score_subdir='post'), store=p['store'], **QUIET).score()
    assert read_bytes(post, 'predict_regions.csv') == want
    assert not os.path.exists(os.path.join(work, 'result_test', 'predict_regions.csv'))
    mrdis.Run3D(dict(cfg, phase='score'), store=p['store'], **QUIET).score()
    assert read_bytes(work, 'result_test', 'predict_regions.csv') == read_bytes(src, 'predict_regions.csv')
    # a missing or mis-shaped input file raises the ValueError that names it
    fn = os.path.join(work, 'result_test', names[1])
    good = np.load(fn)
    for spoil in ('shape', 'dtype', 'missing'):
        if spoil == 'shape':
            np.save(fn, good[:, :, :-1])
        elif spoil == 'dtype':
            np.save(fn, good.astype(np.int16))
        else:
            os.remove(fn)
        with pytest.raises(ValueError, match=names[1]):
            mrdis.Run3D(dict(cfg, phase='postprocess'), store=p['store'], **QUIET).postprocess()
    os.remove(os.path.join(post, names[0]))
    with pytest.raises(ValueError, match=names[0]):
        mrdis.Run3D(dict(cfg, phase='score', score_subdir='post'), store=p['store'], **QUIET).score()
    with pytest.raises(ValueError):
        mrdis.Run3D(dict(cfg, phase='postprocess', post_et_min_voxels=5, dataset_name='ZeroDose'), store=p['store'], **QUIET)
