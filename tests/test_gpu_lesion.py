"""Lesion-wise scores and binary dilation on the GPU: the kernels of csrc/mrdis_lesion.hip (lesion.region_planes, lesion.dilate, lesion.lesion_match,
lesion.lesion_expand) behind mrdis.dilate3d and mrdis.lesion_scores.

The oracle is the numpy two-step procedure of tests/lesion_check.py (checked against scipy.ndimage on the CPU by tests/test_lesion_cpu.py).
Integer outputs -- dilated volumes, counts, lesion rows -- are held EQUAL to it; the float64 scores within 1e-12 relative (the host sums the
same float64 terms in the same order; only sqrt and the divisions could differ, by an ulp).  Launch counters prove which kernels ran.

Shapes: (2, 12, 10, 70) and (3, 9, 17, 130) cross the 4 x 4 x 64 tile of csrc/mrdis_cc.hip, the 8 x 8 x 64 tile of the dilation with its halo
of one voxel, and -- D = 70 and 130 are no multiples of four, P = 8400 is and 19890 is not -- both the dword and the byte form of every
byte store; (1, 1, 1, 1) and (1, 1, 9, 70) are the degenerate ones."""
import os
import shutil

import numpy as np
import pytest
import torch

import lesion_check as lc

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SHAPE_A, SHAPE_B = (2, 12, 10, 70), (3, 9, 17, 130)
REL = 1e-12


@pytest.fixture(scope='module')
def mrdis():
    import mrdis as m
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def lesion_counts(mrdis):
    c = mrdis.hip.launch_counts()
    return {k: c[k] for k in mrdis.hip.LESION_FAMILIES + ('cclabel', 'regsurf', 'surfhist')}


def close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = np.isnan(want) | (np.abs(got - want) <= REL * np.abs(want))
    assert ok.all(), (got[~ok], want[~ok])


def check(mrdis, labels, targets, has_target=None, table=None, **kw):
    """mrdis.lesion_scores == the oracle on every output; `table`: the targets argument the package gets instead of the uint8 volume"""
    okw = {k: v for k, v in kw.items() if k not in ('max_items', 'crop')}
    want = lc.lesion_scores(labels, targets, has_target=has_target, **okw)
    got = mrdis.lesion_scores(dev(labels), dev(targets) if table is None else table, **kw)
    assert got['names'] == ('wt', 'tc', 'et')
    for key in ('counts', 'lesions'):
        assert got[key].dtype == torch.int64 and not got[key].is_cuda
        assert np.array_equal(got[key].numpy(), want[key]), (key, got[key].numpy(), want[key])
    for key in ('lesion_dice', 'lesion_hd95', 'lesion_dice_each', 'lesion_hd95_each'):
        assert got[key].dtype == torch.float64 and not got[key].is_cuda
        close(got[key].numpy(), want[key])
    return got


def blank(shape):
    return np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)


# ----------------------------------------------------------------------------------------------- dilate3d
def np_dilate_batch(vol, n, c):
    return np.stack([lc.dilate(v, n, c) for v in vol])


@pytest.mark.parametrize('c', (6, 18, 26))
def test_dilate3d_equals_the_oracle(mrdis, c):
    rng = np.random.RandomState(c)
    for shape in (SHAPE_A, SHAPE_B, (1, 1, 1, 1), (1, 1, 9, 70), (1, 8, 8, 64), (1, 9, 9, 65)):
        mask = (rng.rand(*shape) < 0.004).astype(np.uint8)
        mask[0, -1, -1, -1] = 1                                      # a corner voxel: every border at once
        mask[-1, 0, 0, 0] = 1
        for n in (1, 2, 3, 4):
            mrdis.hip.launch_counts(reset=True)
            got = mrdis.dilate3d(dev(mask), iterations=n, connectivity=c)
            assert lesion_counts(mrdis)['dilate'] == n and got.dtype == torch.uint8 and tuple(got.shape) == shape
            assert np.array_equal(got.cpu().numpy(), np_dilate_batch(mask, n, c)), (shape, n)
    flags = (rng.rand(*SHAPE_B) < 0.01) * rng.randint(1, 256, SHAPE_B)           # every bit is a plane of its own
    got = mrdis.dilate3d(dev(flags.astype(np.uint8)), 2, c).cpu().numpy()
    assert np.array_equal(got, np_dilate_batch(flags.astype(np.uint8), 2, c))
    m3 = rng.rand(9, 17, 130) < 0.01                                 # (H, W, D) bool in, (H, W, D) uint8 out
    got = mrdis.dilate3d(dev(m3), 1, c)
    assert tuple(got.shape) == (9, 17, 130) and np.array_equal(got.cpu().numpy(), lc.dilate(m3, 1, c).astype(np.uint8))


def test_dilate3d_is_the_iterated_18_neighbourhood_not_a_ball(mrdis):
    mask = np.zeros((1, 12, 12, 12), np.uint8)
    mask[0, 5, 5, 5] = 1
    got = mrdis.dilate3d(dev(mask), 3, 18).cpu().numpy()[0]
    assert got[8, 8, 5] == 1 and got[7, 7, 7] == 1 and got[2, 2, 5] == 1
    assert got[8, 8, 8] == 0 and got[8, 8, 6] == 0 and int(got.sum()) == int(lc.dilate(mask[0], 3, 18).sum())


def test_dilate3d_does_not_leak_across_samples_or_wrap(mrdis):
    mask = np.zeros(SHAPE_A, np.uint8)
    mask[0, -1, -1, -1] = 1                                          # the last voxel of sample 0: flat neighbour of sample 1's first
    mask[0, 3, 4, 0] = 1                                             # the start of a line: flat neighbour of the line before
    got = mrdis.dilate3d(dev(mask), 3, 26).cpu().numpy()
    assert int(got[1].sum()) == 0 and int(got[0, :, :, :3].sum()) == int(got[0, 0:7, 1:8, :3].sum()) > 0
    assert got[0, 3, 3, -1] == 0 and got[0, 0, 0, 0] == 0 and np.array_equal(got, np_dilate_batch(mask, 3, 26))


def test_refusals_launch_nothing(mrdis):
    mrdis.hip.launch_counts(reset=True)
    with pytest.raises(mrdis.MrdisError, match='unsupported geometry'):
        mrdis.dilate3d(torch.zeros((1, 1025, 1, 1), dtype=torch.uint8, device=DEV))
    with pytest.raises(mrdis.MrdisError, match='unsupported geometry'):
        mrdis.lesion_scores(torch.zeros((1, 1, 1, 1025), dtype=torch.uint8, device=DEV), None)
    with pytest.raises(mrdis.MrdisError):
        mrdis.lesion.dilate(torch.zeros((1, 4, 4, 4), dtype=torch.int32, device=DEV))
    with pytest.raises(mrdis.MrdisError):
        mrdis.lesion.dilate(torch.zeros((1, 4, 4, 8), dtype=torch.uint8, device=DEV)[..., ::2])
    lab = torch.zeros((1, 4, 4, 4), dtype=torch.uint8, device=DEV)
    for kw in ({'dilation': 9}, {'dilation': -1}, {'min_voxels': -1}, {'max_items': 0}):
        with pytest.raises(ValueError):
            mrdis.lesion_scores(lab, lab, **kw)
    for kw in ({'iterations': 0}, {'iterations': 9}, {'connectivity': 8}):
        with pytest.raises(ValueError):
            mrdis.dilate3d(lab, **kw)
    assert sum(mrdis.hip.launch_counts().values()) == 0


# ----------------------------------------------------------------------------------------------- planes
def test_region_planes_agree_with_region_surfaces_through_the_counts(mrdis):
    rng = np.random.RandomState(3)
    labels = rng.choice(np.array([0, 0, 0, 1, 2, 4, 3, 9], np.uint8), size=SHAPE_B)
    targets = rng.choice(np.array([0, 0, 1, 2, 4, 1.5, 8, -1, np.nan], np.float32), size=SHAPE_B).astype(np.float32)
    names, masks = mrdis.region_masks(mrdis.BRATS_REGIONS)
    vol = dev(targets)
    table = torch.tensor([vol.data_ptr() + b * vol[0].numel() * 4 for b in range(SHAPE_B[0])], dtype=torch.int64).to(DEV)
    table[1] = 0                                                     # sample 1 has no ground truth
    mrdis.hip.launch_counts(reset=True)
    planes = mrdis.lesion.region_planes(dev(labels), table, masks)
    assert lesion_counts(mrdis)['dilate'] == 1
    _, counts = mrdis.hip.region_surfaces(dev(labels), table, masks)
    planes, counts = planes.cpu().numpy(), counts.cpu().numpy()
    for r, (_, labs) in enumerate(lc.BRATS_REGIONS):
        p, t = (planes >> r) & 1, (planes >> (4 + r)) & 1
        assert np.array_equal(p.astype(bool), np.isin(labels, labs))
        want_t = lc.region_mask(targets, labs)
        want_t[1] = False
        assert np.array_equal(t.astype(bool), want_t)
        for b in range(SHAPE_B[0]):
            assert [int((p[b] & t[b]).sum()), int(p[b].sum()), int(t[b].sum())] == counts[b, r, :3].tolist()
    assert int((planes & 0x88).sum()) == 0                           # three regions: bits 3 and 7 stay clear


# ----------------------------------------------------------------------------------------------- lesion_scores, hand-built
@pytest.mark.parametrize('axis', (0, 1, 2))
def test_gap_6_is_one_lesion_and_gap_7_two(mrdis, axis):
    labels, targets = blank(SHAPE_A)
    for b, gap in ((0, 6), (1, 7)):
        for start in (1, 1 + 1 + gap):                               # two blobs, one voxel thick along `axis`, `gap` empty voxels between
            idx = [slice(4, 6), slice(4, 6), slice(30, 32)]
            idx[axis] = slice(start, start + 1)
            targets[(b,) + tuple(idx)] = 2
            labels[(b,) + tuple(idx)] = 2
    mrdis.hip.launch_counts(reset=True)
    got = check(mrdis, labels, targets, min_voxels=0)
    assert got['counts'][:, 0].tolist() == [[1, 1, 0, 2, 0], [2, 2, 0, 2, 0]]
    assert got['lesion_dice'][:, 0].tolist() == [1.0, 1.0] and got['lesion_hd95'][:, 0].tolist() == [0.0, 0.0]
    assert got['lesion_dice'][:, 1:].tolist() == [[1.0, 1.0]] * 2    # TC and ET: nothing on either side
    c = lesion_counts(mrdis)
    assert c == {'dilate': 4, 'lesmatch': 1, 'lesexpand': 1, 'cclabel': 6, 'regsurf': 1, 'surfhist': 1}, c


def test_offset_3_3_0_matches_and_3_3_3_is_a_false_positive(mrdis):
    labels, targets = blank(SHAPE_A)
    for b, off in ((0, (3, 3, 0)), (1, (3, 3, 3))):
        targets[b, 4, 4, 20] = 4
        labels[b, 4 + off[0], 4 + off[1], 20 + off[2]] = 4
    got = check(mrdis, labels, targets, min_voxels=1)
    assert got['counts'][0].tolist() == [[1, 1, 0, 1, 0]] * 3        # matched: dice 0 (no overlap), a finite distance
    assert got['counts'][1].tolist() == [[1, 1, 1, 1, 1]] * 3        # missed lesion and one FP
    pen = float(np.sqrt(np.float64(12 * 12 + 10 * 10 + 70 * 70)))
    assert got['lesion_dice'].tolist() == [[0.0] * 3] * 2
    assert got['lesion_hd95'][0].tolist() == [float(np.sqrt(np.float64(18)))] * 3 and got['lesion_hd95'][1].tolist() == [pen] * 3


def test_a_component_bridging_two_lesions_belongs_to_both(mrdis):
    labels, targets = blank(SHAPE_A)
    targets[0, 5, 5, 5:8] = 1
    targets[0, 5, 5, 40:43] = 1
    labels[0, 5, 5, 6:42] = 1                                        # one bar across both
    got = check(mrdis, labels, targets, min_voxels=0)
    assert got['counts'][0, 0].tolist() == [2, 2, 0, 1, 0]
    assert got['lesions'][:2, 4].tolist() == [36, 36] and got['lesions'][:2, 5].tolist() == [2, 2]


def test_a_49_voxel_lesion_leaves_the_denominator_and_its_component_is_no_fp(mrdis):
    labels, targets = blank(SHAPE_A)
    targets[0, 1:8, 1:8, 10] = 2                                     # 49 voxels
    targets[0, 2:7, 2:7, 40:42] = 2                                  # 50 voxels
    labels[0, 1:8, 1:8, 10] = 2
    labels[0, 2:7, 2:7, 41:43] = 2
    got = check(mrdis, labels, targets, min_voxels=50)
    assert got['counts'][0, 0].tolist() == [2, 1, 0, 2, 0] and got['lesions'][:2, 3].tolist() == [49, 50]
    assert got['lesions'][:2, 8].tolist() == [0, 1] and got['lesion_dice'][0, 0].item() == 0.5
    assert check(mrdis, labels, targets, min_voxels=49)['counts'][0, 0].tolist() == [2, 2, 0, 2, 0]


def test_empty_sides_and_a_sample_without_ground_truth(mrdis):
    labels, targets = blank(SHAPE_B)
    targets[0, 2:6, 3:8, 60:70] = 1                                  # sample 0: empty prediction
    labels[1, 2:6, 3:8, 60:70] = 1                                   # sample 1: empty ground truth; sample 2: both empty
    got = check(mrdis, labels, targets)
    pen = float(np.sqrt(np.float64(9 * 9 + 17 * 17 + 130 * 130)))
    assert got['counts'][:, 0].tolist() == [[1, 1, 1, 0, 0], [0, 0, 0, 1, 1], [0, 0, 0, 0, 0]]
    assert got['lesion_dice'][:, 0].tolist() == [0.0, 0.0, 1.0] and got['lesion_hd95'][:, 0].tolist() == [pen, pen, 0.0]
    vol = dev(targets.astype(np.float32))
    table = torch.tensor([vol.data_ptr(), 0, vol.data_ptr() + 2 * vol[0].numel() * 4], dtype=torch.int64).to(DEV)
    got = check(mrdis, labels, targets, has_target=[True, False, True], table=table)
    assert torch.isnan(got['lesion_dice'][1]).all() and torch.isnan(got['lesion_hd95'][1]).all()
    assert got['counts'][1, 0].tolist() == [0, 0, 0, 1, 1]
    got = mrdis.lesion_scores(dev(labels), None)
    assert torch.isnan(got['lesion_dice']).all() and got['lesions'].shape == (0, 9)


def scene(shape, boxes, seed):
    """a ground truth of `boxes` random boxes of labels 1 / 2 / 4 and a prediction made of it: shifted by a voxel, some boxes dropped, specks added"""
    rng = np.random.RandomState(seed)
    B, H, W, D = shape
    targets, labels = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    for b in range(B):
        for _ in range(boxes):
            h, w, d = rng.randint(0, H - 1), rng.randint(0, W - 1), rng.randint(0, D - 1)
            sh, sw, sd = rng.randint(1, 5), rng.randint(1, 5), rng.randint(1, 9)
            lab = rng.choice([1, 2, 4])
            targets[b, h:h + sh, w:w + sw, d:d + sd] = lab
            if rng.rand() < 0.75:
                o = rng.randint(-1, 2, 3)
                labels[b, max(0, h + o[0]):h + o[0] + sh, max(0, w + o[1]):w + o[1] + sw, max(0, d + o[2]):d + o[2] + sd] = rng.choice([1, 2, 4])
        speck = rng.rand(H, W, D) < 0.0015
        labels[b][speck] = rng.choice(np.array([1, 2, 4], np.uint8), size=int(speck.sum()))
    return labels, targets


@pytest.mark.parametrize('boxes', (3, 8, 16))
def test_random_scenes_equal_the_oracle_and_two_runs_are_bit_equal(mrdis, boxes):
    labels, targets = scene(SHAPE_B, boxes, seed=boxes)
    a = check(mrdis, labels, targets, min_voxels=12)
    b = mrdis.lesion_scores(dev(labels), dev(targets), min_voxels=12)
    for key in ('lesion_dice', 'lesion_hd95', 'counts', 'lesions', 'lesion_dice_each', 'lesion_hd95_each'):
        assert a[key].numpy().tobytes() == b[key].numpy().tobytes(), key
    assert int(a['counts'][..., 0].sum()) >= 3 and int(a['counts'][..., 4].sum()) >= 1
    check(mrdis, labels, targets, min_voxels=0, spacing=1.5, dilation=1)


def test_chunks_of_two_lesions_equal_one_chunk(mrdis):
    labels, targets = scene(SHAPE_A, 6, seed=11)
    mrdis.hip.launch_counts(reset=True)
    a = check(mrdis, labels, targets, min_voxels=4, max_items=2)
    n = a['lesions'].shape[0]
    assert n > 4 and lesion_counts(mrdis)['lesexpand'] == (n + 1) // 2 == lesion_counts(mrdis)['regsurf']
    mrdis.hip.launch_counts(reset=True)
    b = mrdis.lesion_scores(dev(labels), dev(targets), min_voxels=4, max_items=64)
    assert lesion_counts(mrdis)['lesexpand'] == 1 and lesion_counts(mrdis)['lesmatch'] == 1
    for key in ('lesion_dice', 'lesion_hd95', 'counts', 'lesions', 'lesion_dice_each', 'lesion_hd95_each'):
        assert a[key].numpy().tobytes() == b[key].numpy().tobytes(), key


def test_cropped_and_whole_volume_scoring_are_bit_equal(mrdis):
    """crop=True scores a chunk inside the bounding box of its masks: the same integers and the same float64 bits, the penalty still from the whole volume"""
    keys = ('lesion_dice', 'lesion_hd95', 'counts', 'lesions', 'lesion_dice_each', 'lesion_hd95_each')
    cases = [scene(SHAPE_B, 8, seed=31), scene(SHAPE_A, 4, seed=32)]
    labels, targets = blank(SHAPE_A)
    targets[0, 0:3, 0:3, 0:5] = 1                                    # a lesion in the corner of the volume: no padding there
    labels[0, 1:4, 0:2, 1:6] = 1
    targets[0, 9:12, 7:10, 64:70] = 4                                # and one in the opposite corner, missed: the penalty
    targets[1, 5:7, 5:7, 30:34] = 2                                  # sample 1: a small box well inside
    labels[1, 5:7, 6:8, 31:36] = 2
    cases.append((labels, targets))
    full = np.zeros(SHAPE_A, np.uint8)
    full[0] = 2
    cases.append((full, full))                                       # the box is the whole volume
    for labels, targets in cases:
        a = check(mrdis, labels, targets, min_voxels=5, max_items=8, crop=True)
        for max_items, crop in ((8, False), (1, True), (1, False)):
            b = mrdis.lesion_scores(dev(labels), dev(targets), min_voxels=5, max_items=max_items, crop=crop)
            for key in keys:
                assert a[key].numpy().tobytes() == b[key].numpy().tobytes(), (key, max_items, crop)
    pen = float(np.sqrt(np.float64(12 * 12 + 10 * 10 + 70 * 70)))
    a = mrdis.lesion_scores(dev(cases[2][0]), dev(cases[2][1]), min_voxels=5, max_items=1)
    assert a['counts'][0, 0].tolist() == [2, 2, 1, 1, 0] and a['lesion_hd95_each'][1].item() == pen


def test_dilation_0_takes_the_components_of_the_ground_truth(mrdis):
    labels, targets = scene(SHAPE_A, 5, seed=5)
    targets[0, 0, 0, 0:2] = 2
    targets[0, 0, 0, 3:5] = 2                                        # one empty voxel between: two lesions at dilation 0, one at 1
    mrdis.hip.launch_counts(reset=True)
    a = check(mrdis, labels, targets, min_voxels=0, dilation=0)
    assert lesion_counts(mrdis)['dilate'] == 1                       # the planes alone
    b = check(mrdis, labels, targets, min_voxels=0, dilation=1)
    assert a['lesions'][:2, 2].tolist() == [0, 3] and b['lesions'][0, 2].item() == 0 and b['lesions'][1, 2].item() != 3


def test_fp32_ground_truth_with_values_outside_every_region(mrdis):
    labels, targets = scene(SHAPE_B, 6, seed=21)
    t32 = targets.astype(np.float32)
    t32[0, 4, 8, 64:70] = 1.5                                        # non-integral: no region, and it cuts whatever box lies there
    t32[1, 2, 2, 2:6] = 9.0
    t32[2, 1, 1, 100] = np.nan
    t32[2, 6, 12, 90:99] = 4.0
    check(mrdis, labels, t32, min_voxels=0, table=dev(t32))
    vol = dev(t32)
    table = torch.tensor([vol.data_ptr() + b * vol[0].numel() * 4 for b in range(3)], dtype=torch.int64).to(DEV)
    check(mrdis, labels, t32, min_voxels=0, table=table)


def test_degenerate_volumes(mrdis):
    one = np.full((1, 1, 1, 1), 4, np.uint8)
    got = check(mrdis, one, one, min_voxels=1)
    assert got['counts'][0].tolist() == [[1, 1, 0, 1, 0]] * 3 and got['lesion_dice'][0].tolist() == [1.0] * 3
    check(mrdis, one, np.zeros_like(one))
    labels, targets = blank((1, 1, 9, 70))                           # one voxel thick
    targets[0, 0, 2:5, 3:9] = 1
    targets[0, 0, 2:5, 16:20] = 2
    targets[0, 0, 7, 60:70] = 4
    labels[0, 0, 3:6, 4:18] = 1
    labels[0, 0, 0, 40] = 2
    got = check(mrdis, labels, targets, min_voxels=0)
    assert got['counts'][0, 0].tolist() == [3, 3, 1, 2, 1]


# ----------------------------------------------------------------------------------------------- the 3-D entry: predict_lesions
CONTRASTS = ['T1', 'T1c', 'T2', 'T2_FLAIR']
RUN_CFG = dict(dataset_name='BraTS', contrast_list=CONTRASTS, batch_size=2, model_name='NVNet3D', init_channels=8, epochs=1, lr=1e-4,
               device='cuda:0', seed=10, predict_stride=16)
POST = dict(post_connectivity=26, post_min_voxels=30, post_keep='all')
LES = dict(predict_lesions=True, lesion_dilation=2, lesion_min_voxels=20)
QUIET = dict(log=lambda *a: None)


def read_bytes(*parts):
    with open(os.path.join(*parts), 'rb') as f:
        return f.read()


def family_delta(mrdis, before):
    after = mrdis.hip.launch_counts()
    return {k: after[k] - before[k] for k in mrdis.hip.LESION_FAMILIES}


@pytest.fixture(scope='module')
def predicted3d(mrdis, tmp_path_factory):
    """one epoch of training on the tiny world of tests/test_gpu_postproc.py (32 x 32 x 123, three served test subjects), then phase predict on
    the same checkpoint with predict_regions and predict_post, without and with predict_lesions"""
    from fixtures_data3d import data3d_volumes, data3d_subjects
    data = data3d_volumes(n_subj=11, H=32, W=32, D=123, contrasts=CONTRASTS, seed=9)
    subj = data3d_subjects(data)
    root = tmp_path_factory.mktemp('lesion')
    for name, part in (('train', subj[:4]), ('val', subj[4:7]), ('test', subj[7:11])):
        (root / f'fold_BraTS_3d_0_{name}_noval.txt').write_text('\n'.join(part) + '\n')
    cfg = dict(RUN_CFG, data_path=str(root), ckpt_path=str(tmp_path_factory.mktemp('ckpt')), predict_regions=True, predict_post=True, **POST)
    store = mrdis.VolumeStore3D.from_arrays(data, DEV)
    mrdis.Run3D(cfg, store=store, **QUIET).train()
    dirs = {}
    for name in ('off', 'on'):
        dirs[name] = str(tmp_path_factory.mktemp(name) / 'ckpt')
        shutil.copytree(cfg['ckpt_path'], dirs[name])
    c0 = mrdis.hip.launch_counts()
    off = mrdis.Run3D(dict(cfg, phase='predict', ckpt_path=dirs['off']), store=store, **QUIET).predict()
    d_off = family_delta(mrdis, c0)
    c1 = mrdis.hip.launch_counts()
    on = mrdis.Run3D(dict(cfg, phase='predict', ckpt_path=dirs['on'], **LES), store=store, **QUIET).predict()
    return dict(cfg=cfg, store=store, data=data, subj=subj[8:11], dirs=dirs, off=off, on=on, d_off=d_off, d_on=family_delta(mrdis, c1))


def listing(base):
    return sorted(os.path.relpath(os.path.join(r, f), base) for r, _, fs in os.walk(base) for f in fs)


def test_predict_lesions_off_launches_nothing_and_on_leaves_every_other_file(mrdis, predicted3d):
    p = predicted3d
    assert p['d_off'] == {'dilate': 0, 'lesmatch': 0, 'lesexpand': 0}
    assert p['d_on']['dilate'] == 4 * (1 + 2) and p['d_on']['lesmatch'] <= 4 and p['d_on']['lesexpand'] >= p['d_on']['lesmatch']      # two batches, raw and cleaned
    off, on = os.path.join(p['dirs']['off'], 'result_test'), os.path.join(p['dirs']['on'], 'result_test')
    assert not [f for f in listing(off) if 'lesion' in f]
    assert listing(on) == sorted(listing(off) + ['predict_lesions.csv', os.path.join('post', 'predict_lesions.csv')])
    for f in listing(off):
        assert read_bytes(on, f) == read_bytes(off, f), f
    assert all(p['on'][k] == v or (v != v and p['on'][k] != p['on'][k]) for k, v in p['off'].items())
    cols = mrdis.lesion.lesion_csv_header().split(',')
    assert set(p['on']) - set(p['off']) == set(cols) | {f'post_{c}' for c in cols}


def test_predict_lesions_csv_rows_equal_lesion_scores(mrdis, predicted3d):
    p = predicted3d
    cols = mrdis.lesion.lesion_csv_header().split(',')
    for sub, prefix in (('', ''), ('post', 'post_')):
        base = os.path.join(p['dirs']['on'], 'result_test', sub)
        lines = open(os.path.join(base, 'predict_lesions.csv')).read().splitlines()
        assert lines[0] == 'subj_id,' + ','.join(cols) and [ln.split(',')[0] for ln in lines[1:]] == p['subj']
        table = []
        for i, sid in enumerate(p['subj']):
            vol = np.load(os.path.join(base, f'{sid}_seg.npy'))
            seg = np.asarray(p['data'][sid + '/seg'], dtype=np.float32)
            res = mrdis.lesion_scores(dev(vol[None]), dev(seg[None]), dilation=2, min_voxels=20)
            assert lines[1 + i].split(',')[1:] == mrdis.lesion.lesion_csv_values(res, 0), sid
            table.append([float(v) for v in lines[1 + i].split(',')[1:]])
        means = np.array(table).mean(0)
        assert all(p['on'][prefix + c] == float(v) for c, v in zip(cols, means))
    assert int(np.array(table)[:, 6].sum()) >= 1                    # there are lesions to score


def test_phase_score_and_postprocess_reproduce_predict_lesions_csv(mrdis, predicted3d, tmp_path):
    p = predicted3d
    src = os.path.join(p['dirs']['on'], 'result_test')
    work = str(tmp_path / 'ckpt')
    os.makedirs(os.path.join(work, 'result_test'))
    names = [f'{s}_seg.npy' for s in p['subj']]
    for n in names:
        shutil.copy(os.path.join(src, n), os.path.join(work, 'result_test', n))
    cfg = dict(p['cfg'], ckpt_path=work, **LES)
    before = mrdis.hip.launch_counts()
    mrdis.Run3D(dict(cfg, phase='postprocess', predict_lesions=False), store=p['store'], **QUIET).postprocess()
    assert family_delta(mrdis, before) == {'dilate': 0, 'lesmatch': 0, 'lesexpand': 0}
    assert not os.path.exists(os.path.join(work, 'result_test', 'post', 'predict_lesions.csv'))
    stat = mrdis.Run3D(dict(cfg, phase='postprocess'), store=p['store'], **QUIET).postprocess()
    for f in listing(os.path.join(src, 'post')):
        assert read_bytes(work, 'result_test', 'post', f) == read_bytes(src, 'post', f), f
    assert stat['ldice_wt'] == p['on']['post_ldice_wt']
    want = read_bytes(work, 'result_test', 'post', 'predict_lesions.csv')
    os.remove(os.path.join(work, 'result_test', 'post', 'predict_lesions.csv'))
    mrdis.Run3D(dict(cfg, phase='score', score_subdir='post'), store=p['store'], **QUIET).score()
    assert read_bytes(work, 'result_test', 'post', 'predict_lesions.csv') == want
    stat = mrdis.Run3D(dict(cfg, phase='score'), store=p['store'], **QUIET).score()
    assert read_bytes(work, 'result_test', 'predict_lesions.csv') == read_bytes(src, 'predict_lesions.csv') and stat['lhd95_et'] == p['on']['lhd95_et']
    before = mrdis.hip.launch_counts()
    os.remove(os.path.join(work, 'result_test', 'predict_lesions.csv'))
    mrdis.Run3D(dict(cfg, phase='score', predict_lesions=False), store=p['store'], **QUIET).score()
    assert family_delta(mrdis, before) == {'dilate': 0, 'lesmatch': 0, 'lesexpand': 0} and not os.path.exists(os.path.join(work, 'result_test', 'predict_lesions.csv'))


# ----------------------------------------------------------------------------------------------- the 2-D entry: seg_lesions
def test_phase_segment_with_seg_lesions(mrdis, tmp_path):
    """Run.segment on a freshly built model (the state of tests/test_gpu_seg2d.py, no training): seg_lesions off launches no lesion kernel and writes
    the files of today; on, every other file keeps its bytes and the new rows equal lesion_scores on the written volumes"""
    import types
    H, W, D, BS, BLK = 64, 64, 24, 8, 3
    names = ['c0', 'c1']
    cfg = dict(mrdis.DEFAULT_CONFIG)
    cfg.update(contrast_list=names, input_height=H, input_width=W, batch_size=BS, block_size=BLK, lambda_recon_y_fused=1.0, out_num_ch=4, dataset_name='BraTS')
    cfg = mrdis.derive_config(cfg, DEV)
    torch.manual_seed(5); np.random.seed(5)
    model = mrdis.build_model(cfg)
    g = np.random.RandomState(6)
    arrays = {f'S0/{c}': g.randn(H, W, D).astype(np.float32) for c in names}
    arrays['S1/c0'] = g.randn(H, W, D).astype(np.float32)           # S1 lacks a contrast and has no ground truth
    seg = np.zeros((H, W, D), np.float32)
    seg[10:30, 12:40, 5:15] = 2
    seg[15:25, 20:30, 8:12] = 4
    seg[50:53, 50:53, 18:20] = 1
    arrays['S0/seg'] = seg
    store = mrdis.VolumeStore.from_arrays(arrays, DEV)
    model.eval()
    with torch.no_grad(), mrdis.ops.mix_cache():                     # level the four logits so that every class is predicted somewhere
        y = mrdis.segment.pattern_logits(model, cfg, (H, W, D), DEV, [store.ptr(f'S0/{c}') for c in names], [[True] * 2], BLK, BS)[0][0]
        model.output_decoder.output.up[1].bias -= y.transpose(0, 1).reshape(4, -1).median(1).values
    model.train()

    def segment(where, **kw):
        run = object.__new__(mrdis.train.Run)
        run.config = dict(cfg, ckpt_path=str(tmp_path / where), seg_patterns='leave_one_out', seg_post=True, seg_post_min_voxels=40, **kw)
        run.model, run.world, run.rank, run.log = model, 1, 0, (lambda *a, **k: None)
        run.loaders = {'test': types.SimpleNamespace(dataset=types.SimpleNamespace(subj_list=['S0', 'S0', 'S1'], store=store))}
        before = mrdis.hip.launch_counts()
        stat = run.segment()
        return stat, family_delta(mrdis, before), os.path.join(run.config['ckpt_path'], 'result_test')
    stat_off, d_off, off = segment('off')
    stat_on, d_on, on = segment('on', seg_lesions=True, seg_lesion_dilation=2, seg_lesion_min_voxels=10)
    assert d_off == {'dilate': 0, 'lesmatch': 0, 'lesexpand': 0} and d_on['dilate'] == 2 * (1 + 2) and d_on['lesmatch'] == 2      # S0 alone, raw and cleaned
    new = ['seg_lesions.csv', 'seg_lesion_patterns.csv']
    assert listing(on) == sorted(listing(off) + new + [os.path.join('seg', 'post', f) for f in new])
    for f in listing(off):
        assert read_bytes(on, f) == read_bytes(off, f), f
    cols = list(mrdis.segment.LESION_COLUMNS)
    pats = ['full', 'no_c0', 'no_c1']
    for base, sub in ((on, 'seg'), (os.path.join(on, 'seg', 'post'), '')):
        lines = open(os.path.join(base, 'seg_lesions.csv')).read().splitlines()
        assert lines[0].split(',') == ['subj_id', 'pattern', 'n_present'] + cols and len(lines) == 1 + 2 * 3
        assert [tuple(ln.split(',')[:3]) for ln in lines[1:]] == [('S0', 'full', '2'), ('S0', 'no_c0', '1'), ('S0', 'no_c1', '1'),
                                                                  ('S1', 'full', '1'), ('S1', 'no_c0', '0'), ('S1', 'no_c1', '1')]
        assert all(ln.split(',')[3:] == ['nan'] * len(cols) for ln in lines[4:])                   # S1: nothing to score against
        plines = open(os.path.join(base, 'seg_lesion_patterns.csv')).read().splitlines()
        assert plines[0].split(',') == ['pattern', 'subjects'] + cols and [ln.split(',')[:2] for ln in plines[1:]] == [[p_, '1'] for p_ in pats]
        for k, name in enumerate(pats):
            vol = np.load(os.path.join(base, sub, name, 'S0_seg.npy'))
            res = mrdis.lesion_scores(dev(vol[None]), dev(seg[None]), dilation=2, min_voxels=10)
            want = mrdis.lesion.lesion_csv_values(res, 0)
            assert lines[1 + k].split(',')[3:] == want, (base, name)
            assert [float(v) for v in plines[1 + k].split(',')[2:]] == [float(v) for v in want]
            if sub == 'seg':
                assert all(stat_on[f'{name}/{c}'] == float(v) for c, v in zip(cols, want))
    assert all(stat_on[k] == v or (v != v and stat_on[k] != stat_on[k]) for k, v in stat_off.items())
