"""CPU-side checks of the missing-modality evaluation (nearest-neighbour / mean modality code): the C ABI of the cosine top-1 search,
the gallery's subject codes and per-subject means, the source-contrast rule, the `eval_info` plumbing of the entry point and the
single-process restriction.  No GPU: the kernel itself is tested in tests/test_gpu_zsearch.py."""
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


def _header_text():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mrdis.h')).read(), flags=re.S)


def test_cosine_top1_is_declared_exported_and_bound(m):
    txt = _header_text()
    for name in ('mrdis_cosine_top1', 'mrdis_cosine_top1_workspace'):
        assert re.search(r'\b' + name + r'\s*\(', txt), name
        assert name in m.hip.EXPORTED_SYMBOLS, name
        assert hasattr(m.hip.load(), name), name
    src = open(os.path.join(ROOT, 'representation-disentanglement_amd', 'csrc', 'Makefile')).read()
    assert 'mrdis_zsearch.hip' in re.search(r'^SRCS\s*=.*$', src, flags=re.M).group(0)


def test_cosine_top1_workspace_query_is_host_only(m):
    lib = m.hip.load()
    assert lib.mrdis_cosine_top1_workspace(115000, 1024, 64) >= 16 + 8 * 64
    assert lib.mrdis_cosine_top1_workspace(1, 37, 1) > 0
    assert lib.mrdis_cosine_top1_workspace(1000, 480, 65) == 0         # at most 64 queries per launch
    assert lib.mrdis_cosine_top1_workspace(0, 480, 8) == 0


def test_zsearch_counter_and_grid_option_are_known(m):
    lib = m.hip.load()
    assert 'zsearch' in m.hip.KERNEL_FAMILIES and lib.mrdis_launch_count(b'zsearch') >= 0
    assert 'zsearch_grid' in m.hip.OPTION_NAMES
    with m.hip.option('zsearch_grid', 7):
        assert m.hip.get_option('zsearch_grid') == 7


def test_invalid_arguments_are_rejected_before_any_launch(m):
    lib = m.hip.load()
    before = lib.mrdis_launch_count(b'zsearch')
    # null pointers, Q out of range, ldg < D: MRDIS_EINVAL, nothing enqueued
    assert lib.mrdis_cosine_top1(None, 8, None, 4, 8, None, None, 1, None, None, None, 0, None) == -1
    assert lib.mrdis_launch_count(b'zsearch') == before


def _gallery(m, subjects_of_rows, names, M=4, D=6, Z=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    N = len(subjects_of_rows)
    return m.ZGallery(torch.rand(N, M, D, generator=g), torch.randn(N, M, Z, generator=g), torch.tensor(subjects_of_rows, dtype=torch.int32),
                      torch.arange(N, dtype=torch.int64), names)


def test_subject_codes(m):
    gal = _gallery(m, [0, 0, 1, 2, 2, 2], ['Subj_a', 'Subj_b', 'Subj_c'])
    assert gal.codes(['Subj_b', 'Subj_a', 'Subj_c', 'Subj_b']) == [1, 0, 2, 1]
    assert gal.codes(['nobody']) == [-1]                                      # a subject outside the gallery excludes nothing
    assert len(gal) == 6


@pytest.mark.parametrize('M,want', [(2, [1, 0]), (4, [1, 0, 1, 2])])
def test_source_contrast_rule(m, M, want):
    """main_missing.py:414: contrast i is searched with the compact s of contrast abs(1 - i)"""
    assert [m.nn_source_contrast(i) for i in range(M)] == want
    assert len({m.nn_source_contrast(i) for i in range(M)}) == (2 if M == 2 else 3)    # kernel launches per batch


def test_mean_z_excludes_the_query_subject(m):
    rows = [0, 0, 1, 2, 2, 2, 1]
    gal = _gallery(m, rows, ['a', 'b', 'c'], seed=3)
    codes = gal.codes(['b', 'a', 'c', 'zz'])
    for i in range(4):
        got = gal.mean_z(codes, i)
        for r, c in enumerate(codes):
            keep = torch.tensor([s != c for s in rows])
            want = gal.z[keep, i].mean(0)                                      # compute_mean_z_by_s over the other subjects' rows
            assert torch.allclose(got[r], want, atol=1e-6, rtol=0), (i, r)


def test_single_subject_gallery_raises(m):
    gal = _gallery(m, [0, 0, 0], ['only'])
    with pytest.raises(ValueError, match='nothing to search'):
        gal.mean_z(gal.codes(['only']), 0)


def test_gallery_save_load_round_trip(m, tmp_path):
    gal = _gallery(m, [0, 1, 1, 0], ['x', 'y'], seed=5)
    p = gal.save(str(tmp_path / 'result_test' / 'z_gallery.pt'))
    back = m.ZGallery.load(p, torch.device('cpu'))
    for k in ('s_compact', 'z', 'subject', 'slice_idx'):
        a, b = getattr(gal, k), getattr(back, k)
        assert a.dtype == b.dtype and torch.equal(a, b), k
    assert back.subjects == gal.subjects


def test_eval_info_config_default_and_yaml(m, tmp_path):
    assert m.DEFAULT_CONFIG['eval_info'] == ''
    p = tmp_path / 'config.yaml'
    p.write_text(yaml.dump({'phase': 'test', 'eval_info': 'nearest_neighbour'}))
    found, cfg = m.load_config_yaml(str(p))
    assert found and cfg['eval_info'] == 'nearest_neighbour'


def test_main_passes_eval_info_to_evaluate(m, tmp_path, monkeypatch):
    """phase: test -> Run.evaluate(phase='test', set_='test', info=config['eval_info'])"""
    seen = {}

    class FakeRun:
        rank = 0

        def __init__(self, config):
            seen['config'] = config

        def evaluate(self, **kw):
            seen['kw'] = kw
            return {'all': 0.0}
    monkeypatch.setattr(m.train, 'Run', FakeRun)
    for info in ('nearest_neighbour', 'mean', ''):
        p = tmp_path / f'config_{info or "plain"}.yaml'
        p.write_text(yaml.dump({'phase': 'test', 'eval_info': info, 'ckpt_root': str(tmp_path / 'ckpt'), 'ckpt_timelabel': 't' + info}))
        m.train.main([str(p)])
        assert seen['kw'] == {'phase': 'test', 'set_': 'test', 'info': info}


def test_unknown_info_is_rejected(m):
    with pytest.raises(ValueError):
        m.EvalStep(None, dict(m.DEFAULT_CONFIG), info='nearest')


def test_info_under_a_process_group_raises(m, tmp_path):
    import torch.distributed as dist
    gal = _gallery(m, [0, 1], ['a', 'b'])
    dist.init_process_group('gloo', init_method=f'file://{tmp_path / "pg"}', rank=0, world_size=1)
    try:
        for info in ('nearest_neighbour', 'mean'):
            with pytest.raises(NotImplementedError, match='process group'):
                m.EvalStep(None, dict(m.DEFAULT_CONFIG), info=info, gallery=gal)
        m.EvalStep(None, dict(m.DEFAULT_CONFIG))                              # the plain evaluation stays available
    finally:
        dist.destroy_process_group()


def test_eval_info_comes_from_the_current_file_not_the_saved_yaml(m, tmp_path):
    """a test run over a training run's directory merges that run's saved config.yaml (main_missing.py:45-51), but eval_info, like phase,
    is a per-invocation choice: the saved '' must not override the current file's 'nearest_neighbour'"""
    base = {'ckpt_root': str(tmp_path / 'ckpt'), 'ckpt_timelabel': 'run0', 'phase': 'test'}
    p = tmp_path / 'config.yaml'
    p.write_text(yaml.dump({**base, 'eval_info': ''}))
    cfg = m.train.setup_config(str(p), device=torch.device('cpu'))
    assert os.path.exists(os.path.join(cfg['ckpt_path'], 'config.yaml')) and cfg['eval_info'] == ''
    p.write_text(yaml.dump({**base, 'eval_info': 'nearest_neighbour', 'lr': 0.5}))
    cfg = m.train.setup_config(str(p), device=torch.device('cpu'))
    assert cfg['eval_info'] == 'nearest_neighbour'
    assert cfg['lr'] == m.DEFAULT_CONFIG['lr']                              # every other saved key still wins, as in the reference
