"""CPU-side checks of the connected-component clean-up (postproc.py, csrc/mrdis_cc.hip): the numpy oracles of tests/postproc_check.py against
a hand-written flood fill and scipy.ndimage.label, `np_clean` on hand-made cases for each rule and each tie, the new configuration keys, the
launch-counter table, the new ABI symbols, the refusals that happen on the host before any launch, and the CSV writer.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from postproc_check import flood_components, np_clean, np_components, offsets, same_partition

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONN = (6, 18, 26)


# ----------------------------------------------------------------------------------------------- the oracle itself
def test_neighbourhood_sizes():
    assert [len(offsets(c)) for c in CONN] == [6, 18, 26]


@pytest.mark.parametrize('c', CONN)
def test_oracle_equals_a_flood_fill(c):
    rng = np.random.RandomState(c)
    for shape in ((1, 1, 1), (1, 1, 6), (6, 1, 1), (2, 3, 4), (5, 4, 6), (6, 6, 6)):
        for density in (0.0, 0.2, 0.35, 0.5, 1.0):
            mask = rng.rand(*shape) < density
            comp, size = np_components(mask, c)
            fcomp, fsize = flood_components(mask, c)
            assert np.array_equal(comp, fcomp) and np.array_equal(size, fsize), (shape, density)
            assert comp.dtype == np.int32 and size.dtype == np.int32 and int(size.sum()) == int(mask.sum())
            idx = np.arange(mask.size).reshape(shape)
            assert np.array_equal(size > 0, comp == idx)


def test_oracle_on_touching_pairs_and_borders():
    edge = np.zeros((3, 3, 3), bool); edge[0, 0, 0] = edge[0, 1, 1] = True
    corner = np.zeros((3, 3, 3), bool); corner[0, 0, 0] = corner[1, 1, 1] = True
    ncomp = lambda m, c: int((np_components(m, c)[1] > 0).sum())
    assert [ncomp(edge, c) for c in CONN] == [2, 1, 1]
    assert [ncomp(corner, c) for c in CONN] == [2, 2, 1]
    wrap = np.zeros((2, 3, 4), bool); wrap[0, 0, 3] = wrap[0, 1, 0] = True      # the end of a D line and the start of the next
    assert [ncomp(wrap, c) for c in CONN] == [2, 2, 2]
    chain = np.zeros((4, 4, 4), bool)                                           # a serpentine: one component whose root is voxel 0
    for h in range(4):
        for w in range(4):
            chain[h, w, :] = True if (h * 4 + w) % 2 == 0 else False
            chain[h, w, 3 if (h * 4 + w) % 4 == 1 else 0] = True
    comp, size = np_components(chain, 6)
    fcomp, fsize = flood_components(chain, 6)
    assert np.array_equal(comp, fcomp) and np.array_equal(size, fsize)


@pytest.mark.parametrize('c', CONN)
def test_oracle_partition_equals_scipy(c):
    ndi = pytest.importorskip('scipy.ndimage')
    rng = np.random.RandomState(10 + c)
    structure = ndi.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[c])
    for shape, density in (((7, 9, 11), 0.2), ((7, 9, 11), 0.35), ((12, 5, 20), 0.5), ((3, 4, 5), 1.0), ((3, 4, 5), 0.0)):
        mask = rng.rand(*shape) < density
        comp, size = np_components(mask, c)
        lab, n = ndi.label(mask, structure=structure)
        assert same_partition(comp, lab) and int((size > 0).sum()) == n, (shape, density)
        assert np.array_equal(np.sort(size[size > 0]), np.sort(np.bincount(lab.reshape(-1))[1:]))


# ----------------------------------------------------------------------------------------------- np_clean, rule by rule
def line_volume(runs, D=32):
    """(1, 1, 1, D) labels: runs = [(start, length, label), ...]"""
    v = np.zeros((1, 1, 1, D), np.uint8)
    for s, n, l in runs:
        v[0, 0, 0, s:s + n] = l
    return v


def test_np_clean_keep_all_thresholds():
    v = line_volume([(0, 1, 1), (3, 3, 2), (8, 4, 4), (20, 5, 1)])
    out, st = np_clean(v)                                            # the defaults change nothing
    assert np.array_equal(out, v) and st.tolist() == [[4, 4, 13, 0, 4, 0]]
    out, st = np_clean(v, min_voxels=1)
    assert np.array_equal(out, v) and st.tolist() == [[4, 4, 13, 0, 4, 0]]
    out, st = np_clean(v, min_voxels=4)                              # size == threshold is kept
    assert np.array_equal(out, line_volume([(8, 4, 4), (20, 5, 1)])) and st.tolist() == [[4, 2, 13, 4, 4, 0]]
    out, st = np_clean(v, min_voxels=6)
    assert not out.any() and st.tolist() == [[4, 0, 13, 13, 0, 0]]


def test_np_clean_keep_largest_and_its_tie():
    v = line_volume([(0, 1, 1), (3, 5, 2), (10, 5, 4), (20, 2, 1)])                    # two components of five voxels: the first wins
    out, st = np_clean(v, keep='largest')
    assert np.array_equal(out, line_volume([(3, 5, 2)])) and st.tolist() == [[4, 1, 13, 8, 0, 0]]
    out, st = np_clean(v, keep='largest', min_voxels=5)
    assert np.array_equal(out, line_volume([(3, 5, 2)])) and st[0, 1] == 1
    out, st = np_clean(v, keep='largest', min_voxels=6)                                # the candidate is too small: nothing is kept
    assert not out.any() and st.tolist() == [[4, 0, 13, 13, 0, 0]]
    empty = np.zeros((1, 2, 2, 2), np.uint8)
    out, st = np_clean(empty, keep='largest', min_voxels=3, et_min_voxels=9)
    assert not out.any() and st.tolist() == [[0, 0, 0, 0, 0, 0]]


def test_np_clean_et_rule():
    v = line_volume([(0, 6, 2), (6, 3, 4), (12, 2, 4)])              # ET: three voxels joined to the oedema, two on their own
    assert np_clean(v, et_min_voxels=5)[1].tolist() == [[2, 2, 11, 0, 5, 0]]           # n == threshold: kept as it is
    out, st = np_clean(v, et_min_voxels=6)
    assert np.array_equal(out, line_volume([(0, 6, 2), (6, 3, 1), (12, 2, 1)])) and st.tolist() == [[2, 2, 11, 0, 5, 1]]
    out, st = np_clean(v, min_voxels=3, et_min_voxels=4)             # n is counted AFTER step 2: only the three joined voxels are left
    assert np.array_equal(out, line_volume([(0, 6, 2), (6, 3, 1)])) and st.tolist() == [[2, 1, 11, 2, 3, 1]]
    out, st = np_clean(v, et_min_voxels=6, et_replace=0)
    assert np.array_equal(out, line_volume([(0, 6, 2)])) and st[0, 5] == 1
    # values that are no foreground pass through and do not bridge; an et_label outside fg is still counted and replaced
    w = line_volume([(0, 2, 1), (2, 1, 9), (3, 2, 1), (6, 1, 255), (8, 1, 3)])
    out, st = np_clean(w, fg=(1, 2, 4), min_voxels=3, et_label=3, et_min_voxels=2, et_replace=2)
    assert np.array_equal(out, line_volume([(2, 1, 9), (6, 1, 255), (8, 1, 2)])) and st.tolist() == [[2, 0, 4, 4, 1, 1]]


def test_np_clean_is_per_sample():
    v = np.concatenate([line_volume([(0, 3, 1)]), line_volume([(0, 2, 1), (5, 1, 4)]), line_volume([])])
    out, st = np_clean(v, min_voxels=2, et_min_voxels=3)
    assert st.tolist() == [[1, 1, 3, 0, 0, 0], [2, 1, 3, 1, 0, 0], [0, 0, 0, 0, 0, 0]]
    assert np.array_equal(out, np.concatenate([line_volume([(0, 3, 1)]), line_volume([(0, 2, 1)]), line_volume([])]))


# ----------------------------------------------------------------------------------------------- configuration
def test_config_keys_defaults_and_refusals():
    import mrdis
    t3 = mrdis.train3d
    want = {'predict_post': False, 'post_connectivity': 26, 'post_min_voxels': 0, 'post_keep': 'all', 'post_et_min_voxels': 0, 'score_subdir': ''}
    cfg = t3.load_config3d()
    for k, v in want.items():
        assert cfg[k] == v and type(cfg[k]) is type(v), k
    assert t3.load_config3d(os.path.join(ROOT, 'config3d.yaml')) == t3.DEFAULT_CONFIG_3D
    assert 'postprocess' in t3.PHASES and 'scores' not in t3.PHASES
    assert t3.load_config3d(None, {'phase': 'postprocess'})['phase'] == 'postprocess'
    ok = t3.load_config3d(None, {'predict_post': True, 'post_connectivity': 6, 'post_min_voxels': 50, 'post_keep': 'largest',
                                 'post_et_min_voxels': 200, 'score_subdir': 'post'})
    assert ok['post_keep'] == 'largest' and ok['score_subdir'] == 'post'
    assert t3.load_config3d(None, {'post_min_voxels': 5, 'dataset_name': 'ZeroDose'})['post_min_voxels'] == 5
    for bad in ({'post_keep': 'biggest'}, {'post_connectivity': 8}, {'post_et_min_voxels': 5, 'dataset_name': 'ZeroDose'}, {'phase': 'scores'},
                {'post_min_voxels': -1}, {'post_et_min_voxels': -2}, {'predict_post': 'yes'}, {'score_subdir': '../elsewhere'},
                {'post_connectivity': True}, {'post_min_voxels': 1.5}):
        with pytest.raises(ValueError):
            t3.load_config3d(None, bad)
    path, ov = t3.parse_argv(['phase=postprocess', 'post_keep=largest', 'post_min_voxels=4', 'score_subdir=post'])
    cfg = t3.load_config3d(path, ov)
    assert cfg['phase'] == 'postprocess' and cfg['post_keep'] == 'largest' and cfg['post_min_voxels'] == 4 and cfg['score_subdir'] == 'post'


# ----------------------------------------------------------------------------------------------- counters and symbols
def test_cc_families():
    import mrdis
    hip = mrdis.hip
    lib = hip.load()
    assert hip.CC_FAMILIES == ('cclabel', 'ccclean')
    assert set(hip.CC_FAMILIES) <= set(hip.launch_counts())
    others = (hip.KERNEL_FAMILIES + hip.VARIANT_FAMILIES + hip.LATENT_FAMILIES + hip.OUTDEC_FAMILIES + hip.CONV3D_FAMILIES + hip.DATA_FAMILIES +
              hip.LOSS3D_FAMILIES + hip.SEGVOL_FAMILIES + hip.SYNTH_FAMILIES + hip.FUSE_FAMILIES + hip.SURFDIST_FAMILIES + hip.ELEM_FAMILIES)
    assert not set(hip.CC_FAMILIES) & set(others)
    for fam in hip.CC_FAMILIES:
        assert lib.mrdis_launch_count(fam.encode()) >= 0, fam
    assert hip.SURFDIST_FAMILIES == ('regsurf', 'edt', 'surfhist') and len(hip.ELEM_FAMILIES) == 12


def test_new_symbols_are_declared_exported_and_bound():
    import mrdis
    txt = open(os.path.join(ROOT, 'include', 'mrdis.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    declared = set(re.findall(r'\b(mrdis_[a-z0-9_]+)\s*\(', txt))
    lib = mrdis.hip.load()
    for name in ('mrdis_cc_label', 'mrdis_cc_clean', 'mrdis_cc_clean_workspace'):
        assert name in declared, f'{name} not declared in include/mrdis.h'
        assert name in mrdis.hip.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None
    assert lib.mrdis_cc_clean_workspace(3) >= 24 and lib.mrdis_cc_clean_workspace(0) == 0
    assert mrdis.components3d is mrdis.postproc.components3d and mrdis.clean_labels is mrdis.postproc.clean_labels
    assert callable(mrdis.hip.cc_label) and callable(mrdis.hip.cc_clean)
    assert 'mrdis_cc.hip' in open(os.path.join(ROOT, 'representation-disentanglement_amd', 'csrc', 'Makefile')).read()


# ----------------------------------------------------------------------------------------------- refusals on the host, before any launch
def test_argument_errors_are_value_errors():
    import mrdis
    vol = torch.zeros((1, 2, 3, 4), dtype=torch.uint8)               # never reaches a kernel: every call below is refused first
    before = mrdis.hip.launch_counts()
    for kw in ({'fg': (1, 8)}, {'fg': (-1,)}, {'fg': (0, 1)}, {'fg': ()}, {'connectivity': 8}, {'connectivity': 4}, {'connectivity': 27}):
        with pytest.raises(ValueError):
            mrdis.components3d(vol, **kw)
        with pytest.raises(ValueError):
            mrdis.clean_labels(vol, **kw)
    for kw in ({'keep': 'biggest'}, {'keep': None}, {'min_voxels': -1}, {'et_min_voxels': -1}, {'et_label': 8}, {'et_label': -1}, {'et_replace': 8},
               {'et_replace': -2}, {'min_voxels': 1.5}):
        with pytest.raises(ValueError):
            mrdis.clean_labels(vol, **kw)
    assert mrdis.hip.launch_counts() == before


def test_unsupported_geometry_is_refused_before_any_launch():
    import mrdis
    hip = mrdis.hip
    lib = hip.load()
    before = hip.launch_counts()
    for shape in ((1, 1, 1, 1025), (1, 1025, 1, 1), (1, 1, 1025, 1), (0, 2, 2, 2), (1, 2, 0, 2)):
        vol = torch.zeros(shape, dtype=torch.uint8)
        with pytest.raises(hip.MrdisError, match='unsupported geometry'):
            mrdis.components3d(vol)
        with pytest.raises(hip.MrdisError, match='unsupported geometry'):
            mrdis.clean_labels(vol, min_voxels=2)
    with pytest.raises(hip.MrdisError, match='unsupported geometry'):
        mrdis.components3d(torch.zeros((1025, 1, 1), dtype=torch.bool))
    # H W D >= 2^31 by geometry only (no such tensor is allocated), and B beyond a grid dimension
    for geom in ((1, 2048, 1024, 1024), (1, 1024, 1024, 2048), (65536, 1, 1, 1), (0, 1, 1, 1), (1, 1, 1, 1025)):
        assert geom[0] < 1 or geom[0] > 65535 or max(geom[1:]) > 1024 or geom[1] * geom[2] * geom[3] >= 2 ** 31
        with pytest.raises(hip.MrdisError, match='unsupported geometry'):
            hip._cc_geometry(*geom, 'test')
        # the library itself: geometry is checked before every pointer, so nothing is touched (MRDIS_EUNSUPPORTED = -2)
        assert lib.mrdis_cc_label(None, 0b10110, 26, None, None, *geom, None) == -2
        assert lib.mrdis_cc_clean(None, None, None, 0, 0, 4, 0, 1, None, None, None, 0, *geom, None) == -2
    assert lib.mrdis_strerror(-2) == b'unsupported geometry'
    hip._cc_geometry(65535, 1024, 1024, 1024, 'test')                 # the largest geometry there is: H W D = 2^30
    assert lib.mrdis_cc_label(None, 0b10110, 26, None, None, 1, 4, 4, 4, None) == -1          # a supported geometry, no buffers: MRDIS_EINVAL
    with pytest.raises(hip.MrdisError):                                # a host tensor is refused, not handed to a kernel
        mrdis.components3d(torch.zeros((2, 2, 2), dtype=torch.uint8))
    with pytest.raises(hip.MrdisError):
        mrdis.components3d(torch.zeros((2, 2, 2), dtype=torch.float32))
    assert hip.launch_counts() == before


# ----------------------------------------------------------------------------------------------- the CSV writer
def test_stats_csv_writer(tmp_path):
    import mrdis
    pp = mrdis.postproc
    fn = tmp_path / 'postprocess.csv'
    stats = torch.tensor([[3, 1, 40, 7, 5, 1], [0, 0, 0, 0, 0, 0]], dtype=torch.int32)
    pp.write_stats_csv(str(fn), ['s1', 's2'], stats)
    assert fn.read_text() == 'subj_id,components,kept,foreground,removed,et_voxels,et_replaced\ns1,3,1,40,7,5,1\ns2,0,0,0,0,0,0\n'
    pp.write_stats_csv(str(fn), ['s9'], np.array([[1, 2, 3, 4, 5, 0]], dtype=np.int32))
    assert fn.read_text().splitlines()[1] == 's9,1,2,3,4,5,0'
    assert pp.stats_csv_header().split(',')[1:] == ['components', 'kept', 'foreground', 'removed', 'et_voxels', 'et_replaced']
    assert len(pp.STATS_COLUMNS) == 6
    with pytest.raises(ValueError):
        pp.write_stats_csv(str(fn), ['a', 'b'], stats[:1])
