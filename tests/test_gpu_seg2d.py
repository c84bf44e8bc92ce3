"""Whole-subject 2-D segmentation per missing-contrast pattern on the MI355X (phase: segment): the two kernels of csrc/mrdis_seg2d.hip against
the numpy float64 restatement of the rules (tests/seg2d_check.py: this package's own convention), and `segment_volumes` / `Run.segment` / the
entry point end to end on the smallest model (64 x 64, depth 24).

One view is exact: the label is an argmax over the logits themselves.  Two views compare everywhere except where the float64 top-two gap of the
mean probability is below seg2d_check.TAU (1e-5, about 70 times the fp32 rounding of the rule), and at most seg2d_check.CAP (0.1 %) of a
case's voxels may be excluded that way; tests/test_seg2d_cpu.py shows on the same seeds that a plain fp32 evaluation meets both."""
import os

import numpy as np
import pytest
import torch
import yaml

import seg2d_check as SC

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
FILL = 0xAB


def cl(x):
    return x.contiguous(memory_format=torch.channels_last)


def plant_ties(y):
    """equal small integers in 2, 3 and 4 channels at fixed pixels of every sample (C permitting): the lowest class must win"""
    C = y.shape[1]
    y[:, :, 0, 0] = 2.0                                                      # all C channels tie -> class 0
    y[:, :, 0, 1] = -1.0
    y[:, -2:, 0, 1] = 3.0                                                    # the last two tie -> class C - 2
    if C >= 3:
        y[:, :, 1, 0] = -2.0
        y[:, -3:, 1, 0] = 1.0                                                # the last three tie -> class C - 3
    return y


# --------------------------------------------------------------------------- label_planes, one view
ONE_VIEW_SHAPES = {
    'base': (5, 4, 33, 37),              # H W odd: ragged tiles
    'aligned': (5, 4, 32, 36),
    'c2': (5, 2, 33, 37),                # C < 4: 4-byte loads
    'c3': (5, 3, 33, 37),
    'tiles': (2, 4, 40, 52),             # 2080 pixels: three 1024-pixel tiles per sample, the last ragged
}


@pytest.mark.parametrize('n_sets', [1, 3, 16])
@pytest.mark.parametrize('s0', [0, 4, 8])
@pytest.mark.parametrize('shape', list(ONE_VIEW_SHAPES))
def test_label_planes_one_view_is_exact(mrdis, shape, s0, n_sets):
    B, C, H, W = ONE_VIEW_SHAPES[shape]
    D = SC.BASE['D']
    sets = [plant_ties(SC.make_logits(7 * len(shape) + 100 * s + s0, B, C, H, W)) for s in range(n_sets)]
    views = [[cl(y.to(DEV))] for y in sets]
    for relabel in (False, True):
        planes = torch.full((n_sets, D, H, W), FILL, dtype=torch.uint8, device=DEV)
        before = mrdis.hip.launch_counts()
        out = mrdis.hip.seg2d_label_planes(views, [0], planes, s0, relabel=relabel)
        after = mrdis.hip.launch_counts()
        assert out is planes
        assert after['seg2dlabels'] == before['seg2dlabels'] + 1 and after['seg2dfinish'] == before['seg2dfinish']
        got = planes.cpu().numpy()
        for s, y in enumerate(sets):
            want = SC.place(np.full((D, H, W), FILL, dtype=np.uint8), SC.labels_one_view(y.numpy(), 0, relabel), s0)
            assert np.array_equal(got[s], want), (shape, s0, s, relabel, int((got[s] != want).sum()))
            lab = got[s, s0:s0 + B]
            assert (lab[:, 0, 0] == 0).all() and (lab[:, 0, 1] == C - 2).all()                 # the planted ties: the lowest class
            if C >= 3:
                assert (lab[:, 1, 0] == C - 3).all()
            assert set(np.unique(lab)) <= ({0, 1, 2, 4} if relabel else {0, 1, 2, 3})
        if C == 4 and relabel:
            assert (got[:, s0:s0 + B] == 4).any() and not (got[:, s0:s0 + B] == 3).any()


def test_label_planes_one_flipped_view(mrdis):
    """a single view with a flip code is read at the mirrored pixel"""
    B, C, H, W = ONE_VIEW_SHAPES['base']
    y = SC.make_logits(55, B, C, H, W)
    for code in (1, 2):
        planes = torch.zeros((1, B, H, W), dtype=torch.uint8, device=DEV)
        mrdis.hip.seg2d_label_planes([[cl(y.to(DEV))]], [code], planes, 0)
        assert np.array_equal(planes[0].cpu().numpy(), SC.labels_one_view(y.numpy(), code))


# --------------------------------------------------------------------------- label_planes, two views
@pytest.mark.parametrize('name,flips,seed', SC.TWO_VIEW_CASES, ids=[c[0] for c in SC.TWO_VIEW_CASES])
def test_label_planes_two_views(mrdis, name, flips, seed):
    s = SC.BASE
    B, H, W, D, s0 = s['B'], s['H'], s['W'], s['D'], 4
    views = SC.two_view_inputs(seed)
    want, excluded = SC.labels_two_views(views, flips, relabel=True)
    dev_views = [[cl(torch.from_numpy(v).to(DEV)) for v in views]]
    planes = torch.full((1, D, H, W), FILL, dtype=torch.uint8, device=DEV)
    before = mrdis.hip.launch_counts()['seg2dlabels']
    mrdis.hip.seg2d_label_planes(dev_views, flips, planes, s0, relabel=True)
    assert mrdis.hip.launch_counts()['seg2dlabels'] == before + 1
    got = planes[0].cpu().numpy()
    lab = got[s0:s0 + B]
    share = float(excluded.mean())
    wrong = int((lab != want)[~excluded].sum())
    print(f'[seg2d two views {name}] excluded {int(excluded.sum())} of {excluded.size} ({share:.4%}), mismatches outside: {wrong}, '
          f'inside: {int((lab != want)[excluded].sum())}')
    assert share <= SC.CAP
    assert wrong == 0
    assert (got[:s0] == FILL).all() and (got[s0 + B:] == FILL).all()
    again = torch.full((1, D, H, W), FILL, dtype=torch.uint8, device=DEV)
    mrdis.hip.seg2d_label_planes(dev_views, flips, again, s0, relabel=True)
    assert torch.equal(planes, again)                                        # a second run: the same bytes


@pytest.mark.parametrize('C', [2, 3, 4])
def test_two_identical_integer_views_tie_exactly(mrdis, C):
    """identical integer-valued views: both softmaxes are the same numbers, tied channels stay exactly tied, and the lowest class wins"""
    B, H, W = 3, 9, 11
    g = torch.Generator().manual_seed(C)
    y = plant_ties(torch.randint(-3, 4, (B, C, H, W), generator=g).float())
    planes = torch.zeros((2, B, H, W), dtype=torch.uint8, device=DEV)
    v = cl(y.to(DEV))
    mrdis.hip.seg2d_label_planes([[v, v], [v, v.clone()]], [0, 0], planes, 0)
    want = SC.labels_one_view(y.numpy())                                     # the mean of two equal softmaxes orders the classes as the logits do
    assert np.array_equal(planes[0].cpu().numpy(), want) and np.array_equal(planes[1].cpu().numpy(), want)
    assert (want[:, 0, 0] == 0).all() and (want[:, 0, 1] == C - 2).all()


# --------------------------------------------------------------------------- finish
@pytest.mark.parametrize('n_sets', [1, 3])
@pytest.mark.parametrize('HW', [(33, 37), (32, 36), (1, 1)], ids=str)
@pytest.mark.parametrize('D', [1, 13, 155])
def test_finish_is_the_transpose(mrdis, D, HW, n_sets):
    H, W = HW
    g = torch.Generator().manual_seed(D * 100 + H + n_sets)
    planes = torch.randint(0, 256, (n_sets, D, H, W), generator=g, dtype=torch.uint8)
    before = mrdis.hip.launch_counts()
    out = mrdis.hip.seg2d_finish(planes.to(DEV))
    after = mrdis.hip.launch_counts()
    assert after['seg2dfinish'] == before['seg2dfinish'] + 1 and after['seg2dlabels'] == before['seg2dlabels']
    assert tuple(out.shape) == (n_sets, H, W, D) and out.dtype == torch.uint8 and out.is_contiguous()
    assert np.array_equal(out.cpu().numpy(), np.ascontiguousarray(planes.numpy().transpose(0, 2, 3, 1)))


def test_finish_deeper_than_one_chunk(mrdis):
    """D above the 160 planes of one LDS tile: two chunks per pixel tile"""
    planes = torch.randint(0, 256, (2, 170, 5, 7), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    out = mrdis.hip.seg2d_finish(planes.to(DEV))
    assert np.array_equal(out.cpu().numpy(), np.ascontiguousarray(planes.numpy().transpose(0, 2, 3, 1)))


# --------------------------------------------------------------------------- wrapper layout errors
def test_wrappers_refuse_other_layouts(mrdis):
    x = cl(torch.zeros(5, 4, 6, 7, device=DEV))
    planes = torch.zeros(1, 13, 6, 7, dtype=torch.uint8, device=DEV)
    before = mrdis.hip.launch_counts()
    for bad in (lambda: mrdis.hip.seg2d_label_planes([[x.contiguous()]], [0], planes, 3),                  # contiguous, not channels-last
                lambda: mrdis.hip.seg2d_label_planes([[x.half()]], [0], planes, 3),
                lambda: mrdis.hip.seg2d_label_planes([[x, cl(x[:, :, :5])]], [0, 1], planes, 3),           # the views differ in shape
                lambda: mrdis.hip.seg2d_label_planes([[x]], [0], planes[:, :, :, :6], 3),
                lambda: mrdis.hip.seg2d_label_planes([[x]], [0], planes.repeat(2, 1, 1, 1), 3),            # one set, two volumes
                lambda: mrdis.hip.seg2d_label_planes([[x]], [0], planes, 9),
                lambda: mrdis.hip.seg2d_label_planes([[x.cpu()]], [0], planes, 3),
                lambda: mrdis.hip.seg2d_finish(planes.permute(0, 1, 3, 2))):
        with pytest.raises(mrdis.MrdisError):
            bad()
    assert mrdis.hip.launch_counts() == before


# --------------------------------------------------------------------------- end to end
H, W, D, BS, BLK = 64, 64, 24, 8, 3


def make_state(mrdis, M, seed, **kw):
    names = [f'c{i}' for i in range(M)]
    cfg = dict(mrdis.DEFAULT_CONFIG)
    cfg.update(contrast_list=names, input_height=H, input_width=W, batch_size=BS, block_size=BLK, lambda_recon_y_fused=1.0, out_num_ch=4,
               dataset_name='BraTS', **kw)
    cfg = mrdis.derive_config(cfg, DEV)
    torch.manual_seed(seed); np.random.seed(seed)
    model = mrdis.build_model(cfg)
    g = np.random.RandomState(seed + 1)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    inside = (((yy - H / 2 + 0.5) / (0.40 * H)) ** 2 + ((xx - W / 2 + 0.5) / (0.42 * W)) ** 2) <= 1
    arrays = {}
    for s in ('S0', 'S1'):                                                  # S1 lacks its last contrast and has no ground truth
        for c in names:
            if not (s == 'S1' and c == names[-1]):
                arrays[f'{s}/{c}'] = np.where(inside[:, :, None], g.randn(H, W, D).astype(np.float32), np.float32(-10.0))
    arrays['S0/seg'] = (g.randint(0, 5, (H, W, D)) * inside[:, :, None]).astype(np.float32)
    store = mrdis.VolumeStore.from_arrays(arrays, DEV)
    # a freshly initialised decoder favours one class nearly everywhere: level the medians of the four logits on the first batch (the output is
    # linear in the last convolution's bias), so that every class is predicted somewhere and hiding a contrast moves voxels
    model.eval()
    with torch.no_grad(), mrdis.ops.mix_cache():
        y = mrdis.segment.pattern_logits(model, cfg, (H, W, D), DEV, [store.ptr(f'S0/{c}') for c in names], [[True] * M], BLK, BS)[0][0]
        model.output_decoder.output.up[1].bias -= y.transpose(0, 1).reshape(4, -1).median(1).values
    model.train()
    return dict(cfg=cfg, model=model, store=store, names=names, M=M)


def plain_subject(mrdis, st, sid, hidden, keep_logits=False):
    """the plain composition, one pattern at a time: gather with the hidden pointers zeroed, anatomy encoder, reconstruct_output_fused, torch.argmax,
    relabel, planes placed and transposed with torch -> ((H, W, D) uint8 labels, the logits per batch)"""
    model, cfg, store, names, M = st['model'], st['cfg'], st['store'], st['names'], st['M']
    ptrs = [0 if c in hidden else store.ptr(f'{sid}/{c}') for c in names]
    present = np.array([[1.0 if p else 0.0 for p in ptrs]], dtype=np.float32)
    vol = torch.zeros((D, H, W), dtype=torch.uint8, device=DEV)
    logits = []
    was = model.training
    model.eval()
    try:
        with torch.no_grad(), mrdis.ops.mix_cache():
            for s0, B in mrdis.synth_plan(D, BLK, BS):
                rows = torch.tensor([ptrs] * B, dtype=torch.int64).to(DEV)
                idx = torch.arange(s0, s0 + B, dtype=torch.int32).to(DEV)
                none = torch.full((B,), -1, dtype=torch.int32).to(DEV)
                inputs, _, mask_img = mrdis.hip.slice_gather(rows, idx, none, H, W, D, BLK)
                model.premix('enc')
                si = model.compute_anatomy_encoding(mrdis.trainer.split_inputs(inputs, M, 2 * BLK + 1), mask_img)
                mh = np.repeat(present, B, 0)
                y = model.reconstruct_output_fused(si, torch.from_numpy(mh).to(DEV), mh).float()
                lab = torch.argmax(y, dim=1)
                lab[lab == 3] = 4
                vol[s0:s0 + B] = lab.to(torch.uint8)
                if keep_logits:
                    logits.append(y)
    finally:
        model.train(was)
    return vol.permute(1, 2, 0).contiguous(), logits


@pytest.fixture(scope='module')
def st2(mrdis):
    st = make_state(mrdis, 2, seed=5)
    st['res'] = {r['subj_id']: r for r in mrdis.segment_volumes(st['model'], st['cfg'], st['store'], ['S0', 'S1'], 'all')}     # computed once, shared below
    return st


def test_all_patterns_equal_the_plain_composition(mrdis, st2):
    pats = mrdis.seg_patterns(st2['names'], 'all')
    assert [n for n, _ in pats] == ['full', 'no_c0', 'no_c1']
    res = st2['res']['S0']
    assert res['patterns'] == [n for n, _ in pats] and res['present'] == [[True, True], [False, True], [True, False]]
    labels = res['labels']
    assert tuple(labels.shape) == (3, H, W, D) and labels.dtype == torch.uint8 and labels.is_contiguous()
    nbatch = len(mrdis.synth_plan(D, BLK, BS))
    assert nbatch == 3 and [B for _, B in mrdis.synth_plan(D, BLK, BS)] == [8, 8, 2]
    assert res['launches'] == {'seg2dlabels': nbatch, 'seg2dfinish': 1}
    for j, (name, hidden) in enumerate(pats):
        want, _ = plain_subject(mrdis, st2, 'S0', hidden)
        assert torch.equal(labels[j], want), (name, int((labels[j] != want).sum()))
        assert not labels[j][:, :, :BLK].any() and not labels[j][:, :, D - BLK:].any()       # planes nothing predicts hold 0
        assert set(np.unique(labels[j].cpu().numpy())) <= {0, 1, 2, 4}
    print('[seg2d end to end] voxels per label 0 / 1 / 2 / 4:', [[int((labels[j] == v).sum()) for v in (0, 1, 2, 4)] for j in range(3)])
    assert all((labels[0] == v).any() for v in (0, 1, 2, 4))                 # the levelled logits predict every class somewhere
    assert not torch.equal(labels[0], labels[1]) and not torch.equal(labels[0], labels[2]) and not torch.equal(labels[1], labels[2])


def test_shared_encoder_logits_equal_the_per_pattern_logits(mrdis, st2):
    """the condition of the sharing rule: bit for bit, every pattern, every batch, both with and without a flipped view"""
    model, cfg, store, names = st2['model'], st2['cfg'], st2['store'], st2['names']
    ptrs = [store.ptr(f'S0/{c}') for c in names]
    presents = [[True, True], [False, True], [True, False]]
    model.eval()
    try:
        with torch.no_grad(), mrdis.ops.mix_cache():
            for flip in ('', 'h'):
                for s0, B in mrdis.synth_plan(D, BLK, BS):
                    shared = mrdis.segment.pattern_logits(model, cfg, (H, W, D), DEV, ptrs, presents, s0, B, flip, True)
                    each = mrdis.segment.pattern_logits(model, cfg, (H, W, D), DEV, ptrs, presents, s0, B, flip, False)
                    for a, b in zip(shared, each):
                        assert len(a) == len(b) == (2 if flip else 1)
                        for x, y in zip(a, b):
                            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (flip, s0)
            # and they are the logits of the plain composition
            plain = [plain_subject(mrdis, st2, 'S0', hidden, keep_logits=True)[1] for hidden in ([], ['c0'], ['c1'])]
            for k, (s0, B) in enumerate(mrdis.synth_plan(D, BLK, BS)):
                got = mrdis.segment.pattern_logits(model, cfg, (H, W, D), DEV, ptrs, presents, s0, B)
                for j in range(3):
                    assert torch.equal(got[j][0], plain[j][k]), (j, s0)
                assert not torch.equal(got[0][0], got[2][0]) and not torch.equal(got[0][0], got[1][0])     # fusing two maps is not either alone
    finally:
        model.train()


def test_scores_counters_and_training_flag(mrdis, st2):
    model = st2['model'].train()
    mrdis.hip.launch_counts(reset=True)
    res = next(mrdis.segment_volumes(model, st2['cfg'], st2['store'], ['S0'], 'all'))
    cnt = mrdis.hip.launch_counts()
    assert model.training                                                    # the flag is restored
    assert cnt['seg2dlabels'] == 3 and cnt['seg2dfinish'] == 1 and all(cnt[f] == 0 for f in mrdis.hip.CC_FAMILIES + mrdis.hip.SYNTH_FAMILIES)
    assert torch.equal(res['labels'], st2['res']['S0']['labels'])            # a second run: the same bytes
    assert 'post' not in res
    target = torch.from_numpy(np.ascontiguousarray(st2['store'].vols['S0/seg'].permute(1, 2, 0).cpu().numpy())).to(DEV)
    want = mrdis.region_scores(res['labels'], target.unsqueeze(0).repeat(3, 1, 1, 1))
    for k in mrdis.surfdist.SCORE_KEYS:
        assert torch.equal(res['scores'][k], want[k]), k
        assert tuple(res['scores'][k].shape) == (3, 3) and bool(torch.isfinite(res['scores'][k]).all())
    assert torch.equal(res['scores']['counts'], want['counts'])


def test_incomplete_subject_and_missing_ground_truth(mrdis, st2):
    res = st2['res']['S1']                                                   # S1 has c0 only
    assert res['present'] == [[True, False], [False, False], [True, False]]
    assert tuple(res['labels'].shape) == (2, H, W, D) and res['scores'] is None
    assert res['launches'] == {'seg2dlabels': 3, 'seg2dfinish': 1}
    want, _ = plain_subject(mrdis, st2, 'S1', [])
    assert torch.equal(res['labels'][0], want) and torch.equal(res['labels'][1], want)     # 'full' and 'no_c1' see the same subject
    rows = mrdis.segment.score_rows(res)
    assert [(n, k) for n, k, _ in rows] == [('full', 1), ('no_c0', 0), ('no_c1', 1)] and all(np.isnan(v).all() for _, _, v in rows)
    mrdis.hip.launch_counts(reset=True)
    none = next(mrdis.segment_volumes(st2['model'], st2['cfg'], st2['store'], ['S1'], [['c0']]))
    assert none['labels'] is None and none['scores'] is None and none['present'] == [[False, False]]
    cnt = mrdis.hip.launch_counts()
    assert none['launches'] == {'seg2dlabels': 0, 'seg2dfinish': 0} and cnt['fuse'] == 0 and cnt['regsurf'] == 0     # no volume and no launch
    assert mrdis.segment.score_rows(none)[0][:2] == ('no_c0', 0)


def test_flip_view_and_cleaning(mrdis, st2):
    plain = st2['res']['S0']['labels']
    mrdis.hip.launch_counts(reset=True)
    res = next(mrdis.segment_volumes(st2['model'], st2['cfg'], st2['store'], ['S0'], 'all', flip='w',
                                     post={'min_voxels': 30, 'keep': 'all', 'et_min_voxels': 0}))
    cnt = mrdis.hip.launch_counts()
    assert cnt['seg2dlabels'] == 3 and cnt['seg2dfinish'] == 1 and cnt['ccclean'] == 1 and cnt['cclabel'] == mrdis.hip.CC_LABEL_LAUNCHES
    assert tuple(res['labels'].shape) == tuple(plain.shape) and not torch.equal(res['labels'], plain)     # the second view moves some voxels
    assert set(np.unique(res['labels'].cpu().numpy())) <= {0, 1, 2, 4}
    want, stats = mrdis.clean_labels(res['labels'], connectivity=26, min_voxels=30, keep='all', et_min_voxels=0)
    assert torch.equal(res['post'], want) and torch.equal(res['post_stats'], stats)
    target = st2['store'].vols['S0/seg'].permute(1, 2, 0).contiguous().unsqueeze(0).repeat(3, 1, 1, 1)
    for k in mrdis.surfdist.SCORE_KEYS:
        assert torch.equal(res['post_scores'][k], mrdis.region_scores(want, target)[k]), k


def test_three_contrasts_leave_one_out(mrdis):
    st = make_state(mrdis, 3, seed=6)
    pats = mrdis.seg_patterns(st['names'], 'leave_one_out')
    assert [n for n, _ in pats] == ['full', 'no_c0', 'no_c1', 'no_c2']
    res = next(mrdis.segment_volumes(st['model'], st['cfg'], st['store'], ['S0'], 'leave_one_out'))
    assert res['launches'] == {'seg2dlabels': 3, 'seg2dfinish': 1} and tuple(res['labels'].shape) == (4, H, W, D)
    for j, (name, hidden) in enumerate(pats):
        want, _ = plain_subject(mrdis, st, 'S0', hidden)
        assert torch.equal(res['labels'][j], want), (name, int((res['labels'][j] != want).sum()))
    each = next(mrdis.segment_volumes(st['model'], st['cfg'], st['store'], ['S0'], 'leave_one_out', share_encoder=False))
    assert torch.equal(each['labels'], res['labels'])


def test_bf16m_segments_like_the_plain_composition(mrdis):
    try:
        st = make_state(mrdis, 2, seed=7, compute_dtype='bf16m')
        res = next(mrdis.segment_volumes(st['model'], st['cfg'], st['store'], ['S0'], 'all'))
        for j, hidden in enumerate(([], ['c0'], ['c1'])):
            want, _ = plain_subject(mrdis, st, 'S0', hidden)
            assert torch.equal(res['labels'][j], want), (hidden, int((res['labels'][j] != want).sum()))
    finally:
        mrdis.ops.set_compute_dtype('f32')


def test_models_without_an_output_decoder_are_refused(mrdis, st2):
    cfg = dict(mrdis.DEFAULT_CONFIG)
    cfg.update(contrast_list=st2['names'], input_height=H, input_width=W, batch_size=BS)
    cfg = mrdis.derive_config(cfg, DEV)
    torch.manual_seed(1)
    model = mrdis.build_model(cfg)
    before = mrdis.hip.launch_counts()
    with pytest.raises(ValueError, match='lambda_recon_y_fused'):
        next(mrdis.segment_volumes(model, cfg, st2['store'], ['S0']))
    with pytest.raises(ValueError, match='lambda_recon_y_fused'):
        next(mrdis.segment_volumes(st2['model'], dict(st2['cfg'], dataset_name='NCANDA'), st2['store'], ['S0']))
    assert mrdis.hip.launch_counts() == before


def test_entry_point_phase_segment(mrdis, tmp_path):
    """one training epoch on the synthetic set through main(), then phase=segment twice and phase=test: the files, their consistency, identical
    bytes from the second run, and no segmentation launch in the test phase"""
    names = ['T1', 'T2']
    base = dict(contrast_list=names, input_height=H, input_width=W, batch_size=BS, epochs=1, gpu='0', data_source='synthetic', out_num_ch=4,
                lambda_recon_y_fused=1.0, ckpt_root=str(tmp_path / 'ckpt'), ckpt_timelabel='t0', shuffle=False)
    (tmp_path / 'train.yaml').write_text(yaml.dump(base))
    run = mrdis.train.main([str(tmp_path / 'train.yaml')])
    label = os.path.basename(run.config['ckpt_path'])
    later = {**base, 'ckpt_name': 'epoch000.pth.tar', 'ckpt_timelabel': label}
    (tmp_path / 'seg.yaml').write_text(yaml.dump({**later, 'phase': 'segment', 'seg_patterns': 'all', 'seg_set': 'val', 'seg_post': True,
                                                  'seg_post_min_voxels': 20}))

    def read_all(out_dir):
        got = {}
        for root, _, files in os.walk(os.path.join(out_dir, 'seg')):
            for fn in files:
                got[os.path.relpath(os.path.join(root, fn), out_dir)] = open(os.path.join(root, fn), 'rb').read()
        for fn in ('seg_regions.csv', 'seg_patterns.csv'):
            got[fn] = open(os.path.join(out_dir, fn), 'rb').read()
        return got
    mrdis.hip.launch_counts(reset=True)
    run = mrdis.train.main([str(tmp_path / 'seg.yaml')])
    cnt = mrdis.hip.launch_counts()
    out_dir = os.path.join(run.config['ckpt_path'], 'result_val')
    ds = run.loaders['val'].dataset
    subjects = list(dict.fromkeys(str(s) for s in ds.subj_list))
    Hs, Ws, Ds = ds.store.shape
    pats = ['full', 'no_T1', 'no_T2']
    nbatch = len(mrdis.synth_plan(Ds, BLK, BS))
    assert len(subjects) == 2 and cnt['seg2dlabels'] == 2 * nbatch and cnt['seg2dfinish'] == 2 and cnt['ccclean'] == 2
    first = read_all(out_dir)
    for sub in ('seg', os.path.join('seg', 'post')):
        for s in subjects:
            for p in pats:
                v = np.load(os.path.join(out_dir, sub, p, f'{s}_seg.npy'))
                assert v.shape == (Hs, Ws, Ds) and v.dtype == np.uint8 and set(np.unique(v)) <= {0, 1, 2, 4}
                assert not v[:, :, :BLK].any() and not v[:, :, Ds - BLK:].any()
    for base_dir in (out_dir, os.path.join(out_dir, 'seg', 'post')):
        lines = open(os.path.join(base_dir, 'seg_regions.csv')).read().splitlines()
        cols = lines[0].split(',')
        assert cols == ['subj_id', 'pattern', 'n_present'] + list(mrdis.segment.REGION_COLUMNS) and len(lines) == 1 + len(subjects) * len(pats)
        rows = [ln.split(',') for ln in lines[1:]]
        assert [(r[0], r[1]) for r in rows] == [(s, p) for s in subjects for p in pats]
        assert [r[2] for r in rows] == ['2', '1', '1'] * len(subjects)
        vals = {p: np.array([[float(x) for x in r[3:]] for r in rows if r[1] == p]) for p in pats}
        assert all(np.isfinite(v).all() for v in vals.values())
        plines = open(os.path.join(base_dir, 'seg_patterns.csv')).read().splitlines()
        assert plines[0].split(',') == ['pattern', 'subjects'] + list(mrdis.segment.REGION_COLUMNS) and len(plines) == 1 + len(pats)
        for ln, p in zip(plines[1:], pats):
            f = ln.split(',')
            assert f[0] == p and int(f[1]) == len(subjects)
            assert np.array_equal(np.array([float(x) for x in f[2:]]), vals[p].mean(0))      # the means, recomputed from seg_regions.csv
    post = open(os.path.join(out_dir, 'seg', 'post', 'postprocess.csv')).read().splitlines()
    assert post[0] == 'subj_id,pattern,' + ','.join(mrdis.postproc.STATS_COLUMNS) and len(post) == 1 + len(subjects) * len(pats)
    mrdis.train.main([str(tmp_path / 'seg.yaml')])
    assert read_all(out_dir) == first                                        # a second invocation writes identical bytes
    (tmp_path / 'test.yaml').write_text(yaml.dump({**later, 'phase': 'test'}))
    mrdis.hip.launch_counts(reset=True)
    mrdis.train.main([str(tmp_path / 'test.yaml')])
    cnt = mrdis.hip.launch_counts()
    assert all(cnt[f] == 0 for f in mrdis.hip.SEG2D_FAMILIES) and cnt['all'] > 0
