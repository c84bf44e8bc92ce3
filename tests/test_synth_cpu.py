"""CPU-side checks of the whole-subject synthesis (phase: synthesize): the batch plan, the search-source and target rules, the C ABI plumbing
of the two kernels, the option validation, the entry point's dispatch and the single-process restriction.  No GPU: the kernels and the
driver are tested in tests/test_gpu_synth.py."""
import os
import re

import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def m():
    import mrdis
    return mrdis


def test_synth_plan(m):
    assert m.synth_plan(12, 3, 4) == [(3, 4), (7, 2)]
    assert m.synth_plan(12, 3, 6) == [(3, 6)]                             # the centres 3 .. 8 in one full batch
    assert m.synth_plan(7, 3, 4) == [(3, 1)]                              # a volume of exactly one block
    assert m.synth_plan(5, 0, 2) == [(0, 2), (2, 2), (4, 1)]              # b = 0: every slice is a centre
    assert m.synth_plan(155, 3, 32) == [(3, 32), (35, 32), (67, 32), (99, 32), (131, 21)]
    for D, b, n in [(12, 3, 4), (155, 3, 32), (5, 0, 2), (9, 1, 100)]:
        centres = [s0 + r for s0, B in m.synth_plan(D, b, n) for r in range(B)]
        assert centres == list(range(b, D - b))
    with pytest.raises(ValueError):
        m.synth_plan(6, 3, 4)                                             # D < 2b + 1
    with pytest.raises(ValueError):
        m.synth_plan(12, 3, 0)


def test_synth_source(m):
    assert [m.nn_source_contrast(i) for i in range(3)] == [1, 0, 1]
    assert m.synth_source(1, [True, False, True]) == 0                    # abs(1 - 1) = 0 is present
    assert m.synth_source(0, [False, False, True]) == 2                   # abs(1 - 0) = 1 is absent: the lowest present contrast
    assert m.synth_source(1, [False, False, True]) == 2
    assert m.synth_source(0, [False, True, True]) == 1
    assert m.synth_source(3, [True, True, True, False]) == 2
    with pytest.raises(ValueError):
        m.synth_source(0, [False, False])


def test_synth_targets(m):
    assert m.synth_targets([True, True, True], '') == [0, 1, 2]
    assert m.synth_targets([True, False, True], '') == [0, 2]             # without a code for it, the absent contrast is skipped
    assert m.synth_targets([True, False, True], 'nearest_neighbour') == [0, 1, 2]
    assert m.synth_targets([False, False, True], 'mean') == [0, 1]         # contrast 2 has no source but itself
    assert m.synth_targets([False, False, True], '') == []
    assert m.synth_targets([False, False, False], 'mean') == []
    with pytest.raises(ValueError):
        m.synth_targets([True, True], 'nearest')


def test_option_validation(m):
    names = ['T1', 'T1c', 'T2']
    chk = m.synth.check_synth_options
    assert chk(names) == [] and chk(names, 'mean', ['T2', 'T1'], 'mean') == [0, 2] and chk(names, '', 'T1c') == [1]
    with pytest.raises(ValueError, match='block'):
        chk(names, block='median')
    with pytest.raises(ValueError, match='info'):
        chk(names, info='nearest')
    with pytest.raises(ValueError, match='FLAIR'):
        chk(names, drop=['FLAIR'])
    cfg = dict(m.DEFAULT_CONFIG)
    assert (cfg['synth_info'], cfg['synth_drop'], cfg['synth_block'], cfg['synth_set']) == ('', [], 'centre', 'test')
    assert m.synth.default_fill({'norm_type': 'z-score'}) == -10.0 and m.synth.default_fill({'norm_type': 'zscore'}) == -10.0
    assert m.synth.default_fill({'norm_type': 'mean'}) == 0.0
    assert m.synth.covered_planes(12, 3, 'centre') == (3, 8) and m.synth.covered_planes(12, 3, 'mean') == (0, 11)


def test_synthesize_volumes_rejects_bad_options_before_any_work(m):
    cfg = dict(m.DEFAULT_CONFIG, contrast_list=['a', 'b', 'c'])
    for kw in (dict(block='median'), dict(info='nearest'), dict(drop=['d']), dict(info='mean')):      # the last: no gallery
        with pytest.raises(ValueError):
            next(m.synthesize_volumes(None, cfg, None, ['s'], **kw))


def test_kernels_are_declared_exported_bound_and_counted(m):
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mrdis.h')).read(), flags=re.S)
    lib = m.hip.load()
    for name in ('mrdis_synth_accum', 'mrdis_synth_finish'):
        assert re.search(r'\b' + name + r'\s*\(', txt), name
        assert name in m.hip.EXPORTED_SYMBOLS and hasattr(lib, name), name
    src = open(os.path.join(ROOT, 'representation-disentanglement_amd', 'csrc', 'Makefile')).read()
    assert 'mrdis_synth.hip' in re.search(r'^SRCS\s*=.*$', src, flags=re.M).group(0)
    assert m.hip.SYNTH_FAMILIES == ('synthaccum', 'synthfinish') and set(m.hip.SYNTH_FAMILIES) <= set(m.hip.launch_counts())
    for fam in m.hip.SYNTH_FAMILIES:
        assert lib.mrdis_launch_count(fam.encode()) >= 0
    assert int(re.search(r'#define\s+MRDIS_SYNTH_MAX_SRC\s+(\d+)', txt).group(1)) == m.hip.SYNTH_MAX_SRC


def test_invalid_arguments_are_rejected_before_any_launch(m):
    import ctypes
    lib = m.hip.load()
    before = m.hip.launch_counts()
    one = (ctypes.c_void_p * 1)(64)
    assert lib.mrdis_synth_accum(None, 1, 64, 64, 4, 7, 5, 6, 12, 3, 3, 3, None) == -1                 # no source table
    assert lib.mrdis_synth_accum(one, 0, 64, 64, 4, 7, 5, 6, 12, 3, 3, 3, None) == -1                  # n_src outside 1 .. 8
    assert lib.mrdis_synth_accum(one, 9, 64, 64, 4, 7, 5, 6, 12, 3, 3, 3, None) == -1
    assert lib.mrdis_synth_accum(one, 1, 64, 64, 4, 6, 5, 6, 12, 3, 3, 3, None) == -1                  # even C
    assert lib.mrdis_synth_accum(one, 1, 64, 64, 4, 7, 5, 6, 12, 3, 4, 3, None) == -1                  # c_lo > c_hi
    assert lib.mrdis_synth_accum(one, 1, 64, 64, 4, 7, 5, 6, 12, 3, 0, 7, None) == -1                  # c_hi >= C
    assert lib.mrdis_synth_accum(one, 1, 66, 64, 4, 7, 5, 6, 12, 3, 3, 3, None) == -5                  # acc not 4-byte aligned
    assert lib.mrdis_synth_finish(None, 64, 64, 12, 5, 6, 0.0, None) == -1
    assert lib.mrdis_synth_finish(64, 64, 64, 0, 5, 6, 0.0, None) == -1
    assert m.hip.launch_counts() == before
    acc, cnt = torch.zeros(12, 5, 6), torch.zeros(12, dtype=torch.int32)
    x = torch.zeros(4, 7, 5, 6).contiguous(memory_format=torch.channels_last)
    with pytest.raises(m.MrdisError, match='consecutive'):
        m.hip.synth_accum([x], [3, 4, 6, 7], acc, cnt, 3, 3)
    with pytest.raises(m.MrdisError, match='channels-last'):
        m.hip.synth_accum([x.contiguous()], [3, 4, 5, 6], acc, cnt, 3, 3)
    with pytest.raises(m.MrdisError, match='sources'):
        m.hip.synth_accum([], [3, 4, 5, 6], acc, cnt, 3, 3)
    assert m.hip.launch_counts() == before


def test_main_dispatches_phase_synthesize(m, tmp_path, monkeypatch):
    """phase: synthesize -> Run.synthesize(); the synth_* keys reach the run's config from the current file, not from a saved yaml"""
    seen = {}

    class FakeRun:
        rank = 0

        def __init__(self, config):
            seen['config'] = config

        def synthesize(self, **kw):
            seen['kw'] = kw
            return {'rmse': 0.0}

        def evaluate(self, **kw):
            seen['evaluate'] = kw
            return {}
    monkeypatch.setattr(m.train, 'Run', FakeRun)
    base = {'ckpt_root': str(tmp_path / 'ckpt'), 'ckpt_timelabel': 'run0'}
    p = tmp_path / 'config.yaml'
    p.write_text(yaml.dump({**base, 'phase': 'test'}))
    m.train.main([str(p)])                                                  # leaves config.yaml with the synth_* defaults behind
    assert 'evaluate' in seen and 'kw' not in seen
    p.write_text(yaml.dump({**base, 'phase': 'synthesize', 'synth_info': 'mean', 'synth_drop': ['T1c'], 'synth_block': 'mean', 'synth_set': 'val'}))
    m.train.main([str(p)])
    cfg = seen['config']
    assert seen['kw'] == {} and cfg['phase'] == 'synthesize'
    assert (cfg['synth_info'], cfg['synth_drop'], cfg['synth_block'], cfg['synth_set']) == ('mean', ['T1c'], 'mean', 'val')
    assert os.path.basename(cfg['ckpt_path']) == 'run0'                    # like phase test, it works in the named run's directory


def _bare_run(m, **cfg):
    run = object.__new__(m.train.Run)
    run.config = dict(m.DEFAULT_CONFIG, **cfg)
    run.world, run.rank, run.log = 1, 0, (lambda *a, **k: None)
    return run


def test_run_synthesize_validates_its_options(m):
    for kw in (dict(block='median'), dict(info='nearest'), dict(drop=['FLAIR']), dict(set_='all')):
        with pytest.raises(ValueError):
            _bare_run(m).synthesize(**kw)
    with pytest.raises(ValueError, match='block'):
        _bare_run(m, synth_block='median').synthesize()


def test_synthesize_under_a_process_group_raises(m, tmp_path):
    import torch.distributed as dist
    dist.init_process_group('gloo', init_method=f'file://{tmp_path / "pg"}', rank=0, world_size=1)
    try:
        with pytest.raises(NotImplementedError, match='process group'):
            _bare_run(m).synthesize()
    finally:
        dist.destroy_process_group()
