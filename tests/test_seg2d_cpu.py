"""CPU-side checks of the whole-subject 2-D segmentation (phase: segment): the pattern table, the C ABI plumbing of the two kernels, the option
validation, the entry point's dispatch, the single-process restriction, and the two-view tie yardstick of tests/seg2d_check.py on the exact
seeds tests/test_gpu_seg2d.py uses.  No GPU: the kernels and the driver are tested there."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import yaml

import seg2d_check as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def m():
    import mrdis
    return mrdis


# --------------------------------------------------------------------------- patterns
@pytest.mark.parametrize('M', [2, 3, 4])
def test_pattern_counts_names_and_order(m, M):
    names = ['T1', 'T1c', 'T2', 'FLAIR'][:M]
    full = m.seg_patterns(names, 'full')
    loo = m.seg_patterns(names, 'leave_one_out')
    every = m.seg_patterns(names, 'all')
    assert full == [('full', [])]
    assert len(loo) == M + 1 and loo == [('full', [])] + [(f'no_{c}', [c]) for c in names]
    assert len(every) == 2 ** M - 1 and len({n for n, _ in every}) == len(every)
    assert every[:M + 1] == loo                                            # ordered by the number hidden first
    sizes = [len(h) for _, h in every]
    assert sizes == sorted(sizes) and max(sizes) == M - 1
    idx = [tuple(names.index(c) for c in h) for _, h in every]
    for n in range(M):
        same = [i for i in idx if len(i) == n]
        assert same == sorted(same)                                        # then lexicographically by index
    present_sets = {frozenset(names) - frozenset(h) for _, h in every}
    assert len(present_sets) == 2 ** M - 1 and frozenset() not in present_sets      # every non-empty present set, once
    for name, hidden in every:
        assert name == ('no_' + '_'.join(hidden) if hidden else 'full')


def test_explicit_patterns_and_errors(m):
    names = ['T1', 'T1c', 'T2']
    assert m.seg_patterns(names, [['T2', 'T1'], [], ['T1c']]) == [('no_T1_T2', ['T1', 'T2']), ('full', []), ('no_T1c', ['T1c'])]
    assert m.seg_patterns(names, ['T1c']) == [('no_T1c', ['T1c'])]
    assert m.seg_patterns(['a'], 'leave_one_out') == [('full', [])] and m.seg_patterns(['a'], 'all') == [('full', [])]
    for bad in ('every', [['FLAIR']], [['T1', 'T1c', 'T2']], [['T1'], ['T1']], [['T1', 'T1']], [], 3):
        with pytest.raises(ValueError):
            m.seg_patterns(names, bad)
    assert len(m.seg_patterns(['a', 'b', 'c', 'd', 'e'], 'all')) == 31 > m.hip.SEG2D_MAX_SETS      # such a table goes through the kernel in chunks


# --------------------------------------------------------------------------- ABI
def test_kernels_are_declared_exported_bound_and_counted(m):
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mrdis.h')).read(), flags=re.S)
    lib = m.hip.load()
    for name in ('mrdis_seg2d_label_planes', 'mrdis_seg2d_finish'):
        assert re.search(r'\b' + name + r'\s*\(', txt), name
        assert name in m.hip.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert re.search(r'int\s+mrdis_seg2d_label_planes\s*\(\s*const float\* const\* views, int n_sets, int n_views, const int\* flips, '
                     r'unsigned char\* planes,\s*int B, int C, int H,\s*int W, int D, int s0, int relabel, void\* stream\)', txt)
    assert re.search(r'int\s+mrdis_seg2d_finish\s*\(\s*const unsigned char\* planes, unsigned char\* out, int n_sets, int D, int H, int W, '
                     r'void\* stream\)', txt)
    src = open(os.path.join(ROOT, 'representation-disentanglement_amd', 'csrc', 'Makefile')).read()
    assert 'mrdis_seg2d.hip' in re.search(r'^SRCS\s*=.*$', src, flags=re.M).group(0)
    assert m.hip.SEG2D_FAMILIES == ('seg2dlabels', 'seg2dfinish') and set(m.hip.SEG2D_FAMILIES) <= set(m.hip.launch_counts())
    assert not set(m.hip.SEG2D_FAMILIES) & set(m.hip.KERNEL_FAMILIES + m.hip.ELEM_FAMILIES)
    for fam in m.hip.SEG2D_FAMILIES:
        assert lib.mrdis_launch_count(fam.encode()) >= 0
    assert int(re.search(r'#define\s+MRDIS_SEG2D_MAX_SETS\s+(\d+)', txt).group(1)) == m.hip.SEG2D_MAX_SETS == 16
    assert int(re.search(r'#define\s+MRDIS_SEG2D_MAX_VIEWS\s+(\d+)', txt).group(1)) == m.hip.SEG2D_MAX_VIEWS == 2
    assert len(m.hip.OPTION_NAMES) == 28 and len(m.hip.ELEM_FAMILIES) == 12                 # no library option, no dispatch counter added
    assert m.segment_volumes is m.segment.segment_volumes and m.seg_patterns is m.segment.seg_patterns
    from mrdis import train3d
    assert 'subj_id,' + ','.join(m.segment.REGION_COLUMNS) == train3d.region_csv_header()    # the 3-D entry's column order
    assert tuple(k for _, k in m.segment.REGION_CSV_KEYS) == tuple(m.surfdist.SCORE_KEYS)


def test_bad_scalars_are_rejected_before_any_launch(m):
    lib = m.hip.load()
    before = m.hip.launch_counts()
    views = (ctypes.c_void_p * 32)(*([64] * 32))                            # never dereferenced: every call below fails on a scalar
    flips = (ctypes.c_int * 2)(0, 0)
    flip3 = (ctypes.c_int * 2)(0, 3)
    ok = dict(n_sets=1, n_views=1, flips=flips, B=5, C=4, H=6, W=7, D=13, s0=3)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mrdis_seg2d_label_planes(views, a['n_sets'], a['n_views'], a['flips'], 64, a['B'], a['C'], a['H'], a['W'], a['D'], a['s0'], 0, None)
    for kw in (dict(n_sets=0), dict(n_sets=17), dict(n_views=0), dict(n_views=3), dict(C=1), dict(C=5), dict(s0=9), dict(s0=-1), dict(B=0),
               dict(n_views=2, flips=flip3), dict(H=1 << 16, W=1 << 15)):
        assert call(**kw) == -1, kw
    assert lib.mrdis_seg2d_label_planes(None, 1, 1, flips, 64, 5, 4, 6, 7, 13, 3, 0, None) == -1
    for args in ((None, 64, 1, 13, 6, 7), (64, None, 1, 13, 6, 7), (64, 64, 0, 13, 6, 7), (64, 64, 1, 0, 6, 7), (64, 64, 1, 13, 0, 7)):
        assert lib.mrdis_seg2d_finish(*args, None) == -1, args
    assert m.hip.launch_counts() == before


def test_wrappers_refuse_other_layouts_on_the_host(m):
    before = m.hip.launch_counts()
    x = torch.zeros(5, 4, 6, 7).contiguous(memory_format=torch.channels_last)
    planes = torch.zeros(1, 13, 6, 7, dtype=torch.uint8)
    for bad in (lambda: m.hip.seg2d_label_planes([[x.contiguous()]], [0], planes, 3),                      # not channels-last
                lambda: m.hip.seg2d_label_planes([[x.double()]], [0], planes, 3),
                lambda: m.hip.seg2d_label_planes([[x, x[:4]]], [0, 1], planes, 3),                         # the views differ in shape
                lambda: m.hip.seg2d_label_planes([[x]], [0], planes[:, :, :5], 3),
                lambda: m.hip.seg2d_label_planes([[x]], [0], planes.float(), 3),
                lambda: m.hip.seg2d_label_planes([[x]], [0], planes, 9),                                   # s0 + B > D
                lambda: m.hip.seg2d_label_planes([[x]], [3], planes, 3),
                lambda: m.hip.seg2d_label_planes([[x]], [0, 1], planes, 3),
                lambda: m.hip.seg2d_label_planes([], [0], planes, 3),
                lambda: m.hip.seg2d_label_planes([[x]] * 17, [0], planes.repeat(17, 1, 1, 1), 3),
                lambda: m.hip.seg2d_finish(planes.permute(0, 1, 3, 2)),
                lambda: m.hip.seg2d_finish(planes.float())):
        with pytest.raises(m.MrdisError):
            bad()
    assert m.hip.launch_counts() == before


# --------------------------------------------------------------------------- options, entry point
def test_option_validation(m):
    names = ['T1', 'T1c', 'T2']
    chk = m.segment.check_seg_options
    assert chk(names) == ([('full', [])], None)
    pats, post = chk(names, 'leave_one_out', 'w', {'keep': 'largest', 'min_voxels': 4})
    assert len(pats) == 4 and post == {'min_voxels': 4, 'keep': 'largest', 'et_min_voxels': 0}
    assert chk(names, pats)[0] == pats                                       # the pairs pass through
    for kw in (dict(flip='d'), dict(patterns='some'), dict(post={'keep': 'biggest'}), dict(post={'min_voxels': -1}),
               dict(post={'et_min_voxels': 1.5}), dict(patterns=[('full', ['T1'])])):
        with pytest.raises(ValueError):
            chk(names, **kw)
    cfg = dict(m.DEFAULT_CONFIG)
    assert [cfg[k] for k in m.train.SEG_KEYS] == ['full', '', 'test', False, 0, 'all', 0]


def test_segment_volumes_rejects_bad_input_before_any_work(m):
    cfg = dict(m.DEFAULT_CONFIG, contrast_list=['a', 'b', 'c'], dataset_name='BraTS')
    for kw in (dict(patterns='some'), dict(flip='x'), dict(patterns=[['d']]), dict(post={'keep': 'x'})):
        with pytest.raises(ValueError):
            next(m.segment_volumes(None, cfg, None, ['s'], **kw))
    with pytest.raises(ValueError, match='lambda_recon_y_fused'):            # no output decoder
        next(m.segment_volumes(None, cfg, None, ['s']))

    class WithDecoder:
        output_decoder = object()
    with pytest.raises(ValueError, match='lambda_recon_y_fused'):            # not BraTS
        next(m.segment_volumes(WithDecoder(), dict(cfg, dataset_name='NCANDA'), None, ['s']))


def test_main_dispatches_phase_segment(m, tmp_path, monkeypatch):
    """phase: segment -> Run.segment(); the seg_* keys reach the run's config from the current file, not from a saved yaml"""
    seen = {}

    class FakeRun:
        rank = 0

        def __init__(self, config):
            seen['config'] = config

        def segment(self, **kw):
            seen['kw'] = kw
            return {'scored': 0}

        def evaluate(self, **kw):
            seen['evaluate'] = kw
            return {}
    monkeypatch.setattr(m.train, 'Run', FakeRun)
    base = {'ckpt_root': str(tmp_path / 'ckpt'), 'ckpt_timelabel': 'run0'}
    p = tmp_path / 'config.yaml'
    p.write_text(yaml.dump({**base, 'phase': 'test'}))
    m.train.main([str(p)])                                                  # leaves config.yaml with the seg_* defaults behind
    assert 'evaluate' in seen and 'kw' not in seen
    saved = yaml.safe_load(open(os.path.join(seen['config']['ckpt_path'], 'config.yaml')))
    assert saved['seg_patterns'] == 'full' and saved['seg_post'] is False
    now = {'seg_patterns': [['T1c'], ['T1', 'T2']], 'seg_flip': 'w', 'seg_set': 'val', 'seg_post': True, 'seg_post_min_voxels': 8,
           'seg_post_keep': 'largest', 'seg_post_et_min_voxels': 5}
    p.write_text(yaml.dump({**base, 'phase': 'segment', **now}))
    m.train.main([str(p)])
    cfg = seen['config']
    assert seen['kw'] == {} and cfg['phase'] == 'segment'
    assert {k: cfg[k] for k in m.train.SEG_KEYS} == now
    assert os.path.basename(cfg['ckpt_path']) == 'run0'                    # like phase test, it works in the named run's directory


def _bare_run(m, **cfg):
    run = object.__new__(m.train.Run)
    run.config = dict(m.DEFAULT_CONFIG, **cfg)
    run.world, run.rank, run.log = 1, 0, (lambda *a, **k: None)
    return run


def test_run_segment_validates_its_options(m):
    for kw in (dict(patterns='some'), dict(flip='d'), dict(patterns=[['FLAIR']]), dict(set_='all')):
        with pytest.raises(ValueError):
            _bare_run(m).segment(**kw)
    for cfg in (dict(seg_flip='x'), dict(seg_post='yes'), dict(seg_post=True, seg_post_keep='biggest'), dict(seg_post=True, seg_post_min_voxels=-2),
                dict(seg_patterns=[['T1', 'T1']])):
        with pytest.raises(ValueError):
            _bare_run(m, **cfg).segment()


def test_segment_under_a_process_group_raises(m, tmp_path):
    import torch.distributed as dist
    dist.init_process_group('gloo', init_method=f'file://{tmp_path / "pg"}', rank=0, world_size=1)
    try:
        with pytest.raises(NotImplementedError, match='process group'):
            _bare_run(m).segment()
    finally:
        dist.destroy_process_group()


# --------------------------------------------------------------------------- the oracle itself
def test_one_view_oracle_ties_and_relabel():
    y = np.zeros((1, 4, 2, 3), dtype=np.float32)
    y[0, :, 0, 0] = [1, 2, 2, 0]                                             # classes 1 and 2 tie: the lowest wins
    y[0, :, 0, 1] = [0, 0, 0, 5]
    y[0, :, 1, 2] = [3, 3, 3, 3]
    lab = SC.labels_one_view(y, 0, relabel=True)
    assert lab[0, 0, 0] == 1 and lab[0, 0, 1] == 4 and lab[0, 1, 2] == 0 and lab.dtype == np.uint8
    assert SC.labels_one_view(y, 0, relabel=False)[0, 0, 1] == 3
    assert SC.labels_one_view(y, 2)[0, 0, 2] == 1 and SC.labels_one_view(y, 1)[0, 1, 0] == 1   # the flipped view is read at the mirrored pixel


@pytest.mark.parametrize('name,flips,seed', SC.TWO_VIEW_CASES, ids=[c[0] for c in SC.TWO_VIEW_CASES])
def test_two_view_yardstick_holds_for_a_plain_fp32_evaluation(name, flips, seed):
    """both facts the GPU test relies on, for its exact seeds: the excluded share stays under the cap, and outside the excluded voxels a plain
    fp32 evaluation of the rule (standing in for the kernel) agrees with float64 everywhere"""
    views = SC.two_view_inputs(seed)
    lab64, excluded = SC.labels_two_views(views, flips, relabel=True)
    lab32, p32 = SC.labels_two_views_fp32(views, flips, relabel=True)
    p64 = SC.probs_two_views(views, flips)
    err = float(np.abs(p32.astype(np.float64) - p64).max())
    share = float(excluded.mean())
    print(f'[seg2d two views {name}] max |p32 - p64| {err:.3e}  tau {SC.TAU:g}  excluded {int(excluded.sum())} of {excluded.size} ({share:.4%})')
    assert excluded.size == 6105
    assert share <= SC.CAP
    assert err < SC.TAU / 10                                                 # tau is far above the rounding it must absorb
    assert np.array_equal(lab32[~excluded], lab64[~excluded])
    assert set(np.unique(lab64)) <= {0, 1, 2, 4}


def test_small_scale_logits_would_break_the_cap():
    """why the cases use 3 * randn: at 0.05 * randn the near-ties exceed 0.1 % of the voxels"""
    s = SC.BASE
    views = [SC.make_logits(101, s['B'], s['C'], s['H'], s['W'], scale=0.05).numpy(), SC.make_logits(1101, s['B'], s['C'], s['H'], s['W'], scale=0.05).numpy()]
    _, excluded = SC.labels_two_views(views, (0, 1))
    assert excluded.mean() > SC.CAP
