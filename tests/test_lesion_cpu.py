"""CPU-side checks of the lesion-wise scores (lesion.py, csrc/mrdis_lesion.hip): the numpy oracle of tests/lesion_check.py against scipy.ndimage,
rule 6 (`lesion_scores_from_rows`) on hand-built integers, the ABI tables, the config keys, the csv files and the refusals of the binding.
No kernel launches here; tests/test_gpu_lesion.py runs the kernels against the same oracle."""
import os
import re

import numpy as np
import pytest
import torch

import lesion_check as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('mrdis_region_planes', 'mrdis_dilate_workspace', 'mrdis_dilate', 'mrdis_lesion_match', 'mrdis_lesion_expand')


@pytest.fixture(scope='module')
def m():
    import mrdis
    return mrdis


# ----------------------------------------------------------------------------------------------- the oracle against scipy.ndimage
def volumes():
    rng = np.random.RandomState(0)
    out = [rng.rand(7, 9, 11) < d for d in (0.02, 0.1, 0.35)]
    hand = np.zeros((9, 8, 20), bool)
    hand[0, 0, 0] = hand[8, 7, 19] = hand[4, 4, 10] = True
    hand[2:4, 2:5, 3:6] = True
    out += [hand, np.zeros((3, 3, 3), bool), np.ones((2, 3, 4), bool), np.ones((1, 1, 1), bool)]
    return out


def test_oracle_dilation_and_components_equal_scipy():
    ndi = pytest.importorskip('scipy.ndimage')
    structs = {6: ndi.generate_binary_structure(3, 1), 18: ndi.generate_binary_structure(3, 2), 26: np.ones((3, 3, 3), bool)}
    assert int(structs[18].sum()) == 19 and len(lc.OFFSETS[18]) == 18 and len(lc.OFFSETS[6]) == 6 and len(lc.OFFSETS[26]) == 26
    for vol in volumes():
        for c, st in structs.items():
            for n in (1, 2, 3):
                assert np.array_equal(lc.dilate(vol, n, c), ndi.binary_dilation(vol, st, iterations=n)), (vol.shape, c, n)
            lab, n = ndi.label(vol, st)
            comp = lc.components(vol, c)
            assert np.array_equal(comp >= 0, vol) and len(np.unique(comp[vol])) == n
            for i in range(1, n + 1):                                # one id per scipy label: the smallest flat index of its voxels
                assert (comp[lab == i] == np.flatnonzero((lab == i).reshape(-1))[0]).all()
    bits = (np.random.RandomState(1).rand(5, 6, 7) < 0.1) * np.uint8(0x91)       # a uint8 volume dilates bit by bit
    for bit in (0x01, 0x10, 0x80):
        assert np.array_equal((lc.dilate(bits.astype(np.uint8), 2, 18) & bit) != 0, ndi.binary_dilation((bits & bit) != 0, structs[18], iterations=2))


def test_the_two_step_lesions_are_the_components_of_the_dilated_ground_truth():
    """rule 2 of lesion_scores, proven on the oracle: label, dilate each component, merge == label(dilate(T)); T_L = T and L"""
    ndi = pytest.importorskip('scipy.ndimage')
    st18, full = ndi.generate_binary_structure(3, 2), np.ones((3, 3, 3), bool)
    rng = np.random.RandomState(4)
    for density, n in ((0.004, 3), (0.01, 2), (0.03, 1), (0.01, 0)):
        t = rng.rand(12, 14, 30) < density
        got = lc.lesions_two_step(t, n)
        grown = ndi.binary_dilation(t, st18, iterations=n) if n else t
        lab, count = ndi.label(grown, full)
        assert len(got) == count
        ids = sorted(int(np.flatnonzero((lab == i).reshape(-1))[0]) for i in range(1, count + 1))
        assert [g[0] for g in got] == ids
        for lid, mask, tl in got:
            i = lab.reshape(-1)[lid]
            assert np.array_equal(mask, lab == i) and np.array_equal(tl, t & (lab == i))


def test_oracle_pair_scores_equal_scipy_distances():
    ndi = pytest.importorskip('scipy.ndimage')
    rng = np.random.RandomState(2)
    for _ in range(4):
        s, t = np.zeros((10, 11, 12), bool), np.zeros((10, 11, 12), bool)
        for m_ in (s, t):
            h, w, d = rng.randint(0, 6, 3)
            m_[h:h + rng.randint(2, 5), w:w + rng.randint(2, 5), d:d + rng.randint(2, 6)] = True
        dice, hd, ints = lc.pair_scores(s, t, spacing=2.0)
        assert ints[:3] == [int(t.sum()), int(s.sum()), int((s & t).sum())] and dice == 2.0 * ints[2] / (ints[0] + ints[1])
        ss, ts = s & ~ndi.binary_erosion(s, ndi.generate_binary_structure(3, 1), border_value=0), t & ~ndi.binary_erosion(t, ndi.generate_binary_structure(3, 1), border_value=0)
        assert np.array_equal(ss, lc.surface(s)) and np.array_equal(ts, lc.surface(t))
        ks = []
        for a, b in ((ts, ss), (ss, ts)):
            d2 = np.sort(np.rint(ndi.distance_transform_edt(~b)[a] ** 2).astype(np.int64))
            ks.append(next(int(k) for i, k in enumerate(d2) if 20 * int((d2 <= k).sum()) >= 19 * len(d2)))
        assert ints[3:] == ks and hd == 2.0 * np.sqrt(np.float64(max(ks)))
    empty = np.zeros((3, 4, 5), bool)
    full = np.ones((3, 4, 5), bool)
    pen = float(np.sqrt(np.float64(50)))
    assert lc.pair_scores(empty, empty) == (1.0, 0.0, [0, 0, 0, 0, 0])
    assert lc.pair_scores(empty, full) == (0.0, pen, [60, 0, 0, 0, 0]) and lc.pair_scores(full, empty) == (0.0, pen, [0, 60, 0, 0, 0])
    assert lc.pair_scores(full, full)[:2] == (1.0, 0.0)


def test_oracle_lesion_scores_on_a_hand_built_volume():
    labels, targets = np.zeros((1, 12, 12, 40), np.uint8), np.zeros((1, 12, 12, 40), np.uint8)
    targets[0, 2:6, 2:6, 2:6] = 2                                    # 64 voxels, predicted exactly
    labels[0, 2:6, 2:6, 2:6] = 2
    targets[0, 8, 8, 30:33] = 2                                      # 3 voxels: below min_voxels, touched by a component
    labels[0, 8, 8, 34] = 2
    labels[0, 0, 0, 20] = 2                                          # a false positive
    got = lc.lesion_scores(labels, targets, min_voxels=50)
    assert got['counts'][0].tolist() == [[2, 1, 0, 3, 1], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]
    pen = np.sqrt(np.float64(12 * 12 + 12 * 12 + 40 * 40))
    assert got['lesion_dice'][0].tolist() == [0.5, 1.0, 1.0] and got['lesion_hd95'][0].tolist() == [float((0.0 + pen) / 2), 0.0, 0.0]
    assert got['lesions'][:, [0, 1, 3, 4, 5, 8]].tolist() == [[0, 0, 64, 64, 64, 1], [0, 0, 3, 1, 0, 0]]


# ----------------------------------------------------------------------------------------------- rule 6 on hand-built integers
def test_rule_6_on_hand_built_rows(m):
    f = m.lesion_scores_from_rows
    #        b  r  id   T   S   I  kt ks kept
    rows = [[0, 0, 5, 60, 50, 40, 4, 9, 1],
            [0, 0, 90, 10, 10, 10, 0, 0, 0],                         # not kept: leaves the sums and the denominator
            [0, 0, 200, 70, 0, 0, 0, 0, 1],                          # kept and missed
            [1, 1, 7, 55, 55, 55, 0, 0, 1]]
    dice_each = [2 * 40 / 110, 1.0, 0.0, 1.0]
    pen = 1.5 * np.sqrt(np.float64(4 * 4 + 5 * 5 + 6 * 6))
    hd_each = [1.5 * 3.0, 0.0, pen, 0.0]
    counts = np.zeros((3, 2, 5), np.int64)
    counts[0, 0] = [3, 2, 1, 4, 2]
    counts[1, 1] = [1, 1, 0, 1, 0]
    counts[1, 0] = [0, 0, 0, 3, 3]                                   # no lesion, three false positives
    dice, hd = f(rows, dice_each, hd_each, counts, (4, 5, 6), spacing=1.5, has_target=[True, True, False])
    assert dice.dtype == torch.float64 and tuple(dice.shape) == (3, 2) == tuple(hd.shape)
    assert dice[0, 0].item() == (np.float64(2 * 40 / 110) + 0.0) / 4 and hd[0, 0].item() == ((np.float64(4.5) + pen) + 2 * pen) / 4
    assert dice[0, 1].item() == 1.0 and hd[0, 1].item() == 0.0       # |K| + F = 0
    assert dice[1, 0].item() == 0.0 and hd[1, 0].item() == (3 * pen) / 3
    assert dice[1, 1].item() == 1.0 and hd[1, 1].item() == 0.0
    assert torch.isnan(dice[2]).all() and torch.isnan(hd[2]).all()   # no ground truth
    dice, hd = f(np.zeros((0, 9), np.int64), [], [], np.zeros((1, 3, 5), np.int64), (2, 2, 2))
    assert dice.tolist() == [[1.0] * 3] and hd.tolist() == [[0.0] * 3]


# ----------------------------------------------------------------------------------------------- ABI, tables, files
def test_new_entry_points_counters_and_sources_are_listed(m):
    hip = m.hip
    header = open(os.path.join(ROOT, 'include', 'mrdis.h')).read()
    for name in NEW_SYMBOLS:
        assert name in hip.EXPORTED_SYMBOLS and re.search(r'\b' + name + r'\s*\(', header), name
        assert hasattr(hip.load(), name)
    assert hip.LESION_FAMILIES == ('dilate', 'lesmatch', 'lesexpand') and set(hip.LESION_FAMILIES) <= set(hip.LAUNCH_COUNTERS)
    common = open(os.path.join(ROOT, 'representation-disentanglement_amd', 'csrc', 'mrdis_common.h')).read()
    for fam in hip.LESION_FAMILIES:
        assert f'"{fam}"' in common and hip.load().mrdis_launch_count(fam.encode()) >= 0
    assert 'mrdis_lesion.hip' in open(os.path.join(ROOT, 'representation-disentanglement_amd', 'csrc', 'Makefile')).read()
    assert hip.DILATE_MAX_ITERATIONS == 8 == m.lesion.MAX_DILATION and re.search(r'#define\s+MRDIS_DILATE_MAX_ITERATIONS\s+8\b', header)
    lib = hip.load()                                                 # the workspace query is host only
    assert lib.mrdis_dilate_workspace(1, 2, 3, 4, 5) == 0 and lib.mrdis_dilate_workspace(3, 2, 3, 4, 5) == 120
    assert lib.mrdis_dilate_workspace(9, 2, 3, 4, 5) == 0 and lib.mrdis_dilate_workspace(2, 1, 1025, 1, 1) == 0
    assert m.dilate3d is m.lesion.dilate3d and m.lesion_scores is m.lesion.lesion_scores and m.lesion_scores_from_rows is m.lesion.lesion_scores_from_rows


def test_the_lesion_kernels_use_integer_atomics_only():
    src = open(os.path.join(ROOT, 'representation-disentanglement_amd', 'csrc', 'mrdis_lesion.hip')).read()
    code = re.sub(r'//[^\n]*', '', src)
    assert set(re.findall(r'\batomic\w+', code)) == {'atomicAdd', 'atomicOr'} and not re.search(r'\b(float|double)\b', code.replace('const float* tgt', '').replace(
        'reinterpret_cast<const float*>', ''))


def test_config_keys_and_their_refusals(m):
    t3 = m.train3d
    cfg = t3.load_config3d(None, {})
    assert (cfg['predict_lesions'], cfg['lesion_dilation'], cfg['lesion_min_voxels']) == (False, 3, 50)
    text = open(os.path.join(ROOT, 'config3d.yaml')).read()
    for key in ('predict_lesions: false', 'lesion_dilation: 3', 'lesion_min_voxels: 50'):
        assert re.search(r'^' + key + r'\b', text, flags=re.M), key
    ok = t3.load_config3d(None, {'predict_lesions': True, 'lesion_dilation': 0, 'lesion_min_voxels': 0})
    assert ok['predict_lesions'] is True
    for bad in ({'predict_lesions': 'yes'}, {'lesion_dilation': 9}, {'lesion_dilation': -1}, {'lesion_dilation': 1.5}, {'lesion_dilation': True},
                {'lesion_min_voxels': -1}, {'lesion_min_voxels': 2.0}):
        with pytest.raises(ValueError):
            t3.load_config3d(None, bad)
    with pytest.raises(ValueError, match='BraTS only'):
        t3.load_config3d(None, {'predict_lesions': True, 'dataset_name': 'NCANDA'})
    d2 = dict(m.DEFAULT_CONFIG)
    assert [d2[k] for k in m.train.SEG_LESION_KEYS] == [False, 3, 50]
    chk = m.segment.check_lesion_options
    assert chk(None) is None and chk({}) == {'dilation': 3, 'min_voxels': 50} and chk({'dilation': 0, 'min_voxels': 7}) == {'dilation': 0, 'min_voxels': 7}
    for bad in ({'dilation': 9}, {'dilation': -1}, {'dilation': 2.0}, {'min_voxels': -1}, {'min_voxels': True}):
        with pytest.raises(ValueError):
            chk(bad)
    cfg2 = dict(m.DEFAULT_CONFIG, contrast_list=['a', 'b', 'c'], dataset_name='BraTS')
    with pytest.raises(ValueError, match='seg_lesion_dilation'):
        next(m.segment_volumes(None, cfg2, None, ['s'], lesions={'dilation': 11}))


def fake_scores(m, B, seed):
    rng = np.random.RandomState(seed)
    counts = rng.randint(0, 9, (B, 3, 5)).astype(np.int64)
    dice, hd = rng.rand(B, 3), rng.rand(B, 3) * 100
    return {'lesion_dice': torch.from_numpy(dice), 'lesion_hd95': torch.from_numpy(hd), 'counts': torch.from_numpy(counts)}


def test_csv_headers_and_files(m, tmp_path):
    head = m.lesion.lesion_csv_header()
    cols = head.split(',')
    assert cols[:7] == ['ldice_wt', 'ldice_tc', 'ldice_et', 'lhd95_wt', 'lhd95_tc', 'lhd95_et', 'lesions_wt'] and cols[-1] == 'fp_et' and len(cols) == 21
    assert m.segment.LESION_COLUMNS == tuple(cols)
    a, b = fake_scores(m, 2, 0), fake_scores(m, 1, 1)
    b['lesion_dice'][0] = float('nan')
    b['lesion_hd95'][0] = float('nan')
    path = str(tmp_path / 'predict_lesions.csv')
    means = m.train3d.write_lesion_csv(path, ['s0', 's1', 's2'], [a, b])
    lines = open(path).read().splitlines()
    assert lines[0] == 'subj_id,' + head and len(lines) == 4
    row = lines[2].split(',')
    assert row[0] == 's1' and [float(v) for v in row[1:4]] == a['lesion_dice'][1].tolist() and row[7:10] == [str(int(v)) for v in a['counts'][1, :, 0]]
    assert lines[3].split(',')[1:7] == ['nan'] * 6
    assert means['ldice_wt'] == float(np.mean(a['lesion_dice'][:, 0].numpy())) and means['fp_et'] == float(np.mean([a['counts'][0, 2, 4], a['counts'][1, 2, 4], b['counts'][0, 2, 4]]))
    with pytest.raises(ValueError):
        m.train3d.write_lesion_csv(path, ['s0'], [a])
    res = {'patterns': ['full', 'no_a'], 'present': [[True, True], [False, False]], 'lesions': a}
    rows = m.segment.lesion_rows(res)
    assert rows[0][:2] == ('full', 2) and rows[0][2] == m.lesion.lesion_csv_values(a, 0) and rows[1] == ('no_a', 0, ['nan'] * 21)
    assert m.segment.lesion_rows(dict(res, lesions=None))[0][2] == ['nan'] * 21
    means = m.train.Run._write_seg_lesion_csvs(str(tmp_path), ['full', 'no_a'], [('s0',) + r for r in rows])
    lines = open(str(tmp_path / 'seg_lesions.csv')).read().splitlines()
    assert lines[0] == 'subj_id,pattern,n_present,' + head and lines[1].startswith('s0,full,2,') and lines[2] == 's0,no_a,0,' + ','.join(['nan'] * 21)
    lines = open(str(tmp_path / 'seg_lesion_patterns.csv')).read().splitlines()
    assert lines[0] == 'pattern,subjects,' + head and lines[1].startswith('full,1,') and lines[2].startswith('no_a,0,nan')
    assert means['full/ldice_wt'] == a['lesion_dice'][0, 0].item() and np.isnan(means['no_a/fp_et'])


# ----------------------------------------------------------------------------------------------- the binding refuses before any entry point
class Stub:
    """records the compute entry points a wrapper reaches and answers MRDIS_OK; host-only queries go to the real library"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if name.endswith('_workspace'):
            return getattr(self.real, name)

        def record(*args):
            self.calls.append(name)
            return 0
        return record


def test_wrappers_check_every_tensor_before_any_entry_point(m, monkeypatch):
    hip, les = m.hip, m.lesion
    stub = Stub(hip.load())
    monkeypatch.setattr(hip, 'load', lambda path=None: stub)
    monkeypatch.setattr(hip, '_stream', lambda: 0)
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)                # noqa: E731
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32)               # noqa: E731
    vol = (2, 3, 4, 5)
    ops = lambda: dict(planes=u8(*vol), comp_l=i32(6, 3, 4, 5), rank_l=i32(6, 3, 4, 5), comp_p=i32(6, 3, 4, 5), rank_p=i32(6, 3, 4, 5), first_p=i32(6), R=3)   # noqa: E731
    valid = {
        'region_planes': (lambda: dict(labels=u8(*vol), target_ptrs=torch.zeros(2, dtype=torch.int64), region_masks=(22, 18, 16)), ['mrdis_region_planes']),
        'dilate': (lambda: dict(src=u8(*vol), iterations=3, connectivity=18), ['mrdis_dilate']),
        'lesion_match': (lambda: dict(ops(), n_lesions=4, words=2), ['mrdis_lesion_match']),
        'lesion_expand': (lambda: dict(ops(), bits=i32(4, 2), item=i32(4), j0=1, n=3), ['mrdis_lesion_expand']),
    }
    shapes = {'region_planes': [vol], 'dilate': [vol], 'lesion_match': [(4, 2), (4,), (4,), (4,)], 'lesion_expand': [(3, 3, 4, 5)] * 2}
    for name, (make, calls) in valid.items():
        del stub.calls[:]
        out = getattr(les, name)(**make())
        out = [out] if isinstance(out, torch.Tensor) else list(out)
        assert stub.calls == calls and [tuple(t.shape) for t in out] == shapes[name], name
    bad = {
        'region_planes': [('labels', torch.zeros(vol)), ('labels', u8(2, 3, 4, 10)[..., ::2]), ('target_ptrs', torch.zeros(3, dtype=torch.int64)),
                          ('target_ptrs', torch.zeros(2, dtype=torch.int32)), ('region_masks', (1, 2, 3, 4, 5)), ('region_masks', (256,)), ('labels', u8(1, 1, 1, 1025))],
        'dilate': [('src', torch.zeros(vol, dtype=torch.bool)), ('src', u8(3, 4, 5)), ('iterations', 0), ('iterations', 9), ('connectivity', 8), ('src', u8(1, 1025, 1, 1))],
        'lesion_match': [('comp_l', i32(5, 3, 4, 5)), ('rank_p', torch.zeros((6, 3, 4, 5), dtype=torch.int64)), ('first_p', i32(5)), ('R', 5), ('n_lesions', 0),
                         ('words', 0), ('comp_p', i32(6, 3, 4, 10)[..., ::2]), ('planes', torch.zeros(vol))],
        'lesion_expand': [('bits', i32(4)), ('item', i32(3)), ('j0', 2), ('n', 0), ('j0', -1), ('rank_l', i32(6, 3, 4, 4)), ('bits', torch.zeros((4, 2), dtype=torch.int64))],
    }
    n = 0
    for name, muts in bad.items():
        for key, val in muts:
            kw = valid[name][0]()
            kw[key] = val
            del stub.calls[:]
            with pytest.raises(hip.MrdisError):
                getattr(les, name)(**kw)
            assert stub.calls == [], (name, key)
            n += 1
    assert n == 28
    for fn, kw in ((m.dilate3d, dict(mask=u8(*vol), iterations=0)), (m.dilate3d, dict(mask=u8(*vol), connectivity=True)),
                   (m.lesion_scores, dict(labels=u8(*vol), targets=None, dilation=9)), (m.lesion_scores, dict(labels=u8(*vol), targets=None, min_voxels=-1)),
                   (m.lesion_scores, dict(labels=u8(*vol), targets=None, max_items=0)), (m.lesion_scores, dict(labels=u8(*vol), targets=None, dilation=1.0))):
        with pytest.raises(ValueError):
            fn(**kw)
    with pytest.raises(hip.MrdisError, match='unsupported geometry'):
        m.lesion_scores(u8(1, 1, 1, 1025), None)
    with pytest.raises(hip.MrdisError, match='unsupported geometry'):
        m.dilate3d(u8(1, 1025, 1, 1))
    assert stub.calls == []
    tree = __import__('ast').parse(open(os.path.join(ROOT, 'representation-disentanglement_amd', 'lesion.py')).read())
    assert not [n_.lineno for n_ in __import__('ast').walk(tree) if isinstance(n_, __import__('ast').Assert)]      # python -O strips assert: guards are ifs
