"""Host side of the region scoring (surfdist.py, the `predict_regions` / `phase: score` configuration): the ABI tables, and the step from
integer counts and histograms to Dice, sensitivity, specificity and HD95 on hand-built integers.  No GPU."""
import math
import os
import re

import numpy as np
import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('mrdis_region_surfaces', 'mrdis_edt_workspace', 'mrdis_edt_sq', 'mrdis_surface_hist')


@pytest.fixture(scope='module')
def mrdis():
    import mrdis as m
    return m


def test_header_exports_and_binding_table_know_the_new_entries(mrdis):
    header = open(os.path.join(ROOT, 'include', 'mrdis.h')).read()
    lib = mrdis.hip.load()
    for name in SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, re.sub(r'/\*.*?\*/', '', header, flags=re.S)), name
        assert name in mrdis.hip.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert '#define MRDIS_EDT_FAR (1 << 30)' in header
    assert mrdis.hip.SURFDIST_FAMILIES == ('regsurf', 'edt', 'surfhist')
    assert set(mrdis.hip.SURFDIST_FAMILIES) <= set(mrdis.hip.launch_counts())
    for fam in mrdis.hip.SURFDIST_FAMILIES:
        assert lib.mrdis_launch_count(fam.encode()) >= 0
    assert not set(mrdis.hip.SURFDIST_FAMILIES) & set(mrdis.hip.KERNEL_FAMILIES + mrdis.hip.ELEM_FAMILIES)
    assert mrdis.EDT_FAR == mrdis.hip.EDT_FAR == 1 << 30
    assert mrdis.BRATS_REGIONS == (('wt', (1, 2, 4)), ('tc', (1, 4)), ('et', (4,)))
    for name in ('edt3d_sq', 'region_scores', 'scores_from_counts', 'percentile_ranks'):
        assert callable(getattr(mrdis, name))
    import importlib
    alias = importlib.import_module('mrdis')
    assert alias.region_scores is mrdis.region_scores and alias.EDT_FAR == 1 << 30


def test_workspace_query_is_host_only_and_refuses_unsupported_extents(mrdis):
    lib = mrdis.hip.load()
    n = 4 * 240 * 240 * 155
    assert lib.mrdis_edt_workspace(6, 4, 240, 240, 155) == 6 * n * 2 + 6 * n * 4              # uint16 first pass + int32 second pass
    assert lib.mrdis_edt_workspace(1, 1, 1, 1, 1) == 16 + 4
    assert lib.mrdis_edt_workspace(1, 1, 1024, 1024, 1024) > 0
    for bad in ((1, 1, 1025, 4, 4), (1, 1, 4, 1025, 4), (1, 1, 4, 4, 1025), (1, 1, 0, 4, 4), (1, 0, 4, 4, 4), (0, 1, 4, 4, 4), (9, 1, 4, 4, 4)):
        assert lib.mrdis_edt_workspace(*bad) == 0, bad
    assert mrdis.hip.edt_bins(240, 240, 155) == 2 * 239 ** 2 + 154 ** 2 + 1 == 137959


def test_region_masks(mrdis):
    names, masks = mrdis.region_masks(mrdis.BRATS_REGIONS)
    assert names == ('wt', 'tc', 'et') and masks == (0b10110, 0b10010, 0b10000)
    assert mrdis.region_masks([('a', [0, 7])]) == (('a',), (0b10000001,))
    for bad in ([], [('a', [8])], [('a', [-1])], [('a', [])], [(str(i), [1]) for i in range(5)]):
        with pytest.raises(ValueError):
            mrdis.region_masks(bad)


def test_config_accepts_predict_regions_and_phase_score(mrdis):
    t3 = mrdis.train3d
    assert t3.load_config3d(None, {})['predict_regions'] is False
    cfg = t3.load_config3d(None, {'phase': 'predict', 'predict_regions': True})
    assert cfg['predict_regions'] is True and cfg['phase'] == 'predict'
    assert t3.load_config3d(None, {'phase': 'score'})['phase'] == 'score' and 'score' in t3.PHASES
    _, over = t3.parse_argv(['config3d.yaml', 'phase=predict', 'predict_regions=true'])
    assert t3.load_config3d(None, over)['predict_regions'] is True
    with pytest.raises(KeyError):
        t3.load_config3d(None, {'predict_region': True})                              # unknown keys are still refused
    for bad in ({'predict_regions': 'yes'}, {'predict_regions': True, 'dataset_name': 'ZeroDose'}, {'phase': 'score', 'dataset_name': 'ZeroDose'},
                {'phase': 'scores'}):
        with pytest.raises(ValueError):
            t3.load_config3d(None, bad)
    assert t3.load_config3d(None, {'dataset_name': 'ZeroDose'})['predict_regions'] is False   # the default does not touch other datasets
    with open(os.path.join(ROOT, 'config3d.yaml')) as f:
        y = yaml.safe_load(f)
    assert y['predict_regions'] is False and set(y) == set(t3.DEFAULT_CONFIG_3D)
    assert t3.region_csv_header() == ('subj_id,dice_wt,dice_tc,dice_et,sens_wt,sens_tc,sens_et,spec_wt,spec_tc,spec_et,'
                                      'hd95_wt,hd95_tc,hd95_et')


def test_region_csv_rows_and_means(mrdis, tmp_path):
    t3 = mrdis.train3d
    nan = float('nan')
    scores = {'dice': torch.tensor([[0.1, 0.2, 0.3], [0.5, 0.4, 1 / 3]], dtype=torch.float64),
              'sensitivity': torch.tensor([[1.0, 0.0, 0.25], [nan, nan, nan]], dtype=torch.float64),
              'specificity': torch.ones(2, 3, dtype=torch.float64),
              'hd95': torch.tensor([[math.sqrt(2), 3.0, 373.13], [0.0, 1.0, 2.0]], dtype=torch.float64)}
    fn = str(tmp_path / 'r.csv')
    means = t3.write_region_csv(fn, ['a', 'b'], scores)
    rows = open(fn).read().splitlines()
    assert rows[0] == t3.region_csv_header() and len(rows) == 3
    a = rows[1].split(',')
    assert a[0] == 'a' and [float(x) for x in a[1:4]] == [0.1, 0.2, 0.3] and a[10] == repr(math.sqrt(2))
    assert rows[2].split(',')[4:7] == ['nan', 'nan', 'nan'] and rows[2].split(',')[3] == repr(1 / 3)
    assert means['dice_wt'] == pytest.approx(0.3) and means['sens_et'] == 0.25 and means['hd95_tc'] == 2.0       # NaN rows are left out of a mean


# ---------------------------------------------------------------------------------------------- the percentile rule
def rank_of(mrdis, hist, n=None):
    h = torch.tensor(hist, dtype=torch.int32)
    n = torch.tensor(int(h.sum()) if n is None else n)
    return int(mrdis.percentile_ranks(h, n))


def test_percentile_rule_is_the_nearest_rank_in_integers(mrdis):
    """k = the smallest squared distance with 20 cum[k] >= 19 n: the ceil(0.95 n)-th smallest value"""
    assert rank_of(mrdis, [0, 0, 0, 1]) == 3                                    # n = 1: the value itself
    # n = 19: 20 cum >= 361 needs cum = 19 (20 x 18 = 360 falls short): the largest value
    assert rank_of(mrdis, [18, 0, 1]) == 2 and rank_of(mrdis, [19, 0, 0]) == 0
    # n = 20: 20 cum >= 380 is reached at cum = 19: the 19th smallest, the largest one is cut off
    assert rank_of(mrdis, [18, 1, 0, 1]) == 1 and rank_of(mrdis, [19, 0, 0, 1]) == 0 and rank_of(mrdis, [18, 0, 0, 2]) == 3
    # n = 21: 20 cum >= 399 needs cum = 20
    assert rank_of(mrdis, [19, 1, 1]) == 1 and rank_of(mrdis, [19, 0, 2]) == 2
    # n = 100: cum = 95
    assert rank_of(mrdis, [94, 1, 5]) == 1 and rank_of(mrdis, [94, 0, 6]) == 2 and rank_of(mrdis, [95, 0, 5]) == 0
    assert rank_of(mrdis, [7, 0, 0, 0]) == 0 and rank_of(mrdis, [100000] + [0] * 50) == 0          # all mass in bin 0
    assert rank_of(mrdis, [0, 0, 0], n=0) == 0                                  # nothing measured
    # every n up to 60 against the sorted values
    rng = np.random.RandomState(4)
    for n in range(1, 61):
        vals = np.sort(rng.randint(0, 30, n))
        want = int(vals[-(-19 * n // 20) - 1])                                  # the ceil(19 n / 20)-th smallest
        assert rank_of(mrdis, np.bincount(vals, minlength=30).tolist()) == want, n
    # batched rows, each with its own n
    h = torch.tensor([[[18, 1, 0, 1], [0, 0, 0, 1]], [[0, 4, 0, 0], [0, 0, 0, 0]]], dtype=torch.int32)
    assert mrdis.percentile_ranks(h, h.sum(-1)).tolist() == [[1, 3], [1, 0]]


# ---------------------------------------------------------------------------------------------- counts -> scores
def test_scores_from_hand_built_counts(mrdis):
    shape = (4, 5, 10)                                                          # N = 200
    #           I   P    T   sP  sT
    counts = [[[6, 10, 14, 9, 12],                                              # an ordinary region
               [0, 0, 0, 0, 0],                                                 # both empty
               [0, 7, 0, 7, 0],                                                 # ground truth empty (T = 0)
               [0, 0, 5, 0, 5]],                                                # prediction empty
              [[200, 200, 200, 148, 148],                                       # N = T: the region is the whole volume
               [3, 3, 200, 3, 148], [1, 1, 1, 1, 1], [0, 1, 1, 1, 1]]]
    ranks = [[[5, 8], [0, 0], [0, 0], [0, 0]], [[0, 0], [9, 0], [0, 0], [2, 2]]]
    s = mrdis.scores_from_counts(counts, ranks, shape, spacing=1.5)
    for k in ('dice', 'sensitivity', 'specificity', 'hd95'):
        assert s[k].dtype == torch.float64 and tuple(s[k].shape) == (2, 4)
    diag = 1.5 * math.sqrt(16 + 25 + 100)
    assert s['dice'].tolist() == [[12 / 24, 1.0, 0.0, 0.0], [1.0, 6 / 203, 1.0, 0.0]]
    assert s['sensitivity'].tolist() == [[6 / 14, 1.0, 1.0, 0.0], [1.0, 3 / 200, 1.0, 0.0]]            # T = 0: 1
    assert s['specificity'].tolist() == [[(200 - 10 - 14 + 6) / 186, 1.0, 193 / 200, 1.0], [1.0, 1.0, 1.0, 198 / 199]]       # N = T: 1
    assert s['hd95'].tolist() == [[1.5 * math.sqrt(8), 0.0, diag, diag], [0.0, 1.5 * 3.0, 0.0, 1.5 * math.sqrt(2)]]
    # no ground truth for sample 1: NaN in all four, sample 0 as before
    t = mrdis.scores_from_counts(counts, ranks, shape, spacing=1.5, has_target=[True, False])
    for k in ('dice', 'sensitivity', 'specificity', 'hd95'):
        assert torch.equal(t[k][0], s[k][0]) and bool(torch.isnan(t[k][1]).all())
    assert float(mrdis.scores_from_counts([[[0, 0, 9, 0, 9]]], [[[0, 0]]], (240, 240, 155))['hd95']) == pytest.approx(373.13, abs=5e-3)
