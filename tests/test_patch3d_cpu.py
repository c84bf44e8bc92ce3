"""Patch sampling for the 3-D nets, the part that needs no GPU: the numpy oracle (tests/patch3d_check.py) against hand-worked cases, the loader's
draw order, the untouched default path, the binding's refusals on the stub-library pattern of test_hip_contracts_cpu.py, and the config keys."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
import mrdis                                                    # noqa: E402
import patch3d_check as chk                                     # noqa: E402
from test_hip_contracts_cpu import install_stub, meta, put, short, strided, tensors, to, z, COMPUTE      # noqa: E402

hip = mrdis.hip
patch3d = mrdis.patch3d
F32, I32, I64 = torch.float32, torch.int32, torch.int64


# ---------------------------------------------------------------- the oracle against hand-worked cases
def test_pick_ends_and_every_r():
    for n in (1, 2, 3, 7, 33, 1000, 2 ** 31 - 1):
        assert chk.pick(0, n) == 0 and chk.pick(2 ** 32 - 1, n) == n - 1
    for n in (1, 3, 7, 40, 1025):
        for r in range(n):
            u = chk.u_reaching(r, n)
            assert 0 <= u < 2 ** 32 and chk.pick(u, n) == r
            assert r == 0 or chk.pick(u - 1, n) == r - 1               # u is the FIRST draw that reaches r
    assert chk.u_reaching(1, 2) == 2 ** 31 and chk.u_reaching(1, 3) == 1431655766      # ceil(2^32 / 3)
    assert chk.pick(2 ** 31 - 1, 2) == 0 and chk.pick(2 ** 31, 2) == 1


def hand_seg():
    """(2, 3, 4): flat index f = (h 3 + w) 4 + d.  class 1 at f = 1, 6, 23; class 4 at f = 0; class 2 absent"""
    seg = np.zeros((2, 3, 4), np.float32)
    seg.reshape(-1)[[1, 6, 23]] = 1
    seg.reshape(-1)[0] = 4
    return seg


def test_oracle_counts_and_prefix_by_hand():
    seg = hand_seg()
    assert chk.block_counts(seg, (1, 2, 4)).tolist() == [[3, 0, 1]]
    assert chk.prefix_table(seg, (1, 2, 4)).tolist() == [[0, 0, 0], [3, 0, 1]]
    big = np.zeros((3, 10, 100), np.float32)                       # 3000 voxels: blocks of 1024, 1024, 952
    big.reshape(-1)[[0, 1023, 1024, 2999]] = 2
    assert chk.block_counts(big, (2,)).tolist() == [[2], [1], [1]]
    assert chk.prefix_table(big, (2,)).tolist() == [[0], [2], [3], [4]]


def test_oracle_origin_by_hand():
    seg, shape, patch = hand_seg(), (2, 3, 4), (1, 2, 2)
    top = 2 ** 32 - 1
    # uniform: H - PH + 1 = 2, W - PW + 1 = 2, D - PD + 1 = 3 origins per axis
    assert chk.origin(shape, patch, (0, 0, 0, 0, 0))[:4] == (0, 0, 0, -1)
    assert chk.origin(shape, patch, (0, 0, top, top, top))[:4] == (1, 1, 2, -1)
    assert chk.origin(shape, patch, (0, 0, 2 ** 31, 2 ** 31 - 1, chk.u_reaching(1, 3)))[:4] == (1, 0, 1, -1)
    # foreground: present = [class 1 (index 0), class 4 (index 2)]; class 1 voxels in flat order: (0,0,1), (0,1,2), (1,2,3)
    fg = dict(fg=True, seg=seg, classes=(1, 2, 4))
    assert chk.origin(shape, patch, (0, 0, top, top, top), **fg) == (0, 0, 0, 0, (0, 0, 1))            # hc - 0, wc - 1 -> clamp 0, dc - 1 = 0
    assert chk.origin(shape, patch, (0, chk.u_reaching(1, 3), 0, 0, 0), **fg) == (0, 0, 1, 0, (0, 1, 2))
    assert chk.origin(shape, patch, (0, top, 0, 0, 0), **fg) == (1, 1, 2, 0, (1, 2, 3))                # wc - 1 = 1, dc - 1 = 2: both at their upper clamp
    assert chk.origin(shape, patch, (2 ** 31, 0, 5, 5, 5), **fg) == (0, 0, 0, 2, (0, 0, 0))            # second present class: list index 2
    # fall-backs to the uniform rule with the same u_h, u_w, u_d
    uni = chk.origin(shape, patch, (7, 7, top, 0, top))
    assert uni[:4] == (1, 0, 2, -1)
    assert chk.origin(shape, patch, (7, 7, top, 0, top), fg=True, seg=None, classes=(1, 2, 4)) == uni
    assert chk.origin(shape, patch, (7, 7, top, 0, top), fg=True, seg=seg, classes=(1, 2, 4), has_prefix=False) == uni
    assert chk.origin(shape, patch, (7, 7, top, 0, top), fg=True, seg=seg, classes=(2,)) == uni
    assert chk.origin(shape, patch, (7, 7, top, 0, top), fg=False, seg=seg, classes=(1, 2, 4)) == uni
    assert chk.origin((5, 7, 9), (2, 3, 4), (1, 2, 3, 4, 5), centre=True)[:4] == (1, 2, 2, -1)
    with pytest.raises(AssertionError):
        chk.origin(shape, (3, 1, 1), (0,) * 5)


def test_oracle_gather_by_hand():
    v = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    o, patch = (1, 1, 1), (1, 2, 2)
    assert chk.cut(v, o, patch, (False, False, False)).tolist() == [[[17, 18], [21, 22]]]
    assert chk.cut(v, o, patch, (True, False, False)).tolist() == [[[17, 18], [21, 22]]]               # PH = 1: the H mirror is the identity
    assert chk.cut(v, o, patch, (False, True, False)).tolist() == [[[21, 22], [17, 18]]]
    assert chk.cut(v, o, patch, (False, True, True)).tolist() == [[[22, 21], [18, 17]]]
    x, mask = chk.gather_inputs([v, None], o, patch)
    assert x.shape == (2, 1, 2, 2) and mask.tolist() == [1, 0] and not x[1].any()
    # aug: m0 = min(whole-volume minimum 0, 0 for the absent contrast) = 0 -> only a raw 0 becomes -10; none lies in this patch
    x, _ = chk.gather_inputs([v, None], o, patch, aug=True, scale=1.5, shift=0.25)
    assert x[0].tolist() == [[[25.75, 27.25], [31.75, 33.25]]] and (x[1] == -10).all()                 # the absent contrast's zeros equal m0
    w = v.copy(); w[0, 0, 0] = -10                                   # background marker far from the patch: the whole-volume minimum, not the patch's
    x, _ = chk.gather_inputs([w], (0, 0, 0), (1, 1, 2), aug=True, scale=1.0, shift=0.5)
    assert x.tolist() == [[[[-10, 1.5]]]]
    x, _ = chk.gather_inputs([w], o, patch, aug=True, scale=1.0, shift=0.5)
    assert x.min() == 17.5                                           # the patch's own minimum (17) is NOT rewritten
    # two roundings: 3 * (1 + 2^-23) rounds to 3 + 2^-22 + ... in fp32 before the shift is added
    a, sc, sh = np.float32(3), np.float32(1 + 2.0 ** -23), np.float32(2.0 ** -24)
    x, _ = chk.gather_inputs([np.full((1, 1, 2), a), np.full((1, 1, 2), -10, np.float32)], (0, 0, 0), (1, 1, 1), aug=True, scale=sc, shift=sh)
    assert x[0, 0, 0, 0] == np.float32(np.float32(a * sc) + sh) and x[1, 0, 0, 0] == -10
    seg = np.array([[[0, 1, 2, 4]]], np.float32)
    assert chk.gather_targets(seg, (0, 0, 1), (1, 1, 3)).tolist() == [[[1, 2, 3]]]
    assert chk.gather_targets(seg, (0, 0, 1), (1, 1, 3), (False, False, True), K=3).tolist() == [[[[0, 0, 1]]], [[[0, 1, 0]]], [[[1, 0, 0]]]]
    assert chk.gather_targets(seg, (0, 0, 1), (1, 1, 3), relabel=False).tolist() == [[[1, 2, 4]]]
    assert not chk.gather_targets(None, (0, 0, 1), (1, 1, 3), K=2).any()


# ---------------------------------------------------------------- the loader's draws
class RecordingStream:
    """a np.random.RandomState that notes which method made each draw"""

    def __init__(self, seed):
        self.rs, self.calls = np.random.RandomState(seed), []

    def rand(self):
        self.calls.append('rand')
        return self.rs.rand()

    def choice(self, a, n):
        self.calls.append('choice')
        return self.rs.choice(a, n)

    def randint(self, lo, hi, size, dtype):
        self.calls.append(('randint', lo, hi, size, np.dtype(dtype).name))
        return self.rs.randint(lo, hi, size=size, dtype=dtype)


def small_store(n_subj=3, shape=(6, 8, 10)):
    rs = np.random.RandomState(1)
    data = {}
    for s in range(n_subj):
        for c in ('T1', 'T2'):
            data[f's{s}/{c}'] = rs.randn(*shape).astype(np.float32)
        data[f's{s}/seg'] = rs.randint(0, 5, size=shape).astype(np.float32)
    del data['s1/T2']
    return data, mrdis.VolumeStore3D.from_arrays(data, 'cpu')


def test_draw_order_under_a_seeded_stream():
    data, store = small_store()
    RANDINT = ('randint', 0, 2 ** 32, 5, 'uint32')
    for aug, dropoff, fg, flips in ((True, True, 0.5, 'hwd'), (True, False, 0.0, 'd'), (False, True, 1.0, 'h'), (True, True, 0.25, '')):
        ds = mrdis.VolumeDataset3D('BraTS', store, ['s0', 's1', 's2'], contrast_list=['T1', 'T2'], aug=aug, dropoff=dropoff,
                                   patch_size=(2, 4, 4), patch_fg=fg, patch_flips=flips)
        for seed in range(12):
            for idx in range(3):
                rec, twin = RecordingStream(seed), np.random.RandomState(seed)
                m = ds.meta(idx, rec)
                n_present = 1 if idx == 1 else 2
                want = chk.draw_item(twin, n_present, dropoff, aug, fg, flips)
                calls = list(rec.calls)
                if dropoff and n_present > 1:                          # 1. the reference's drop-off draws
                    assert calls.pop(0) == 'rand'
                    if m[3] >= 0:
                        assert calls.pop(0) == 'choice'
                if fg > 0:                                             # 2. the foreground draw
                    assert calls.pop(0) == 'rand'
                assert calls.pop(0) == RANDINT                         # 3. the five uint32, one call
                assert calls == ['rand'] * ((len(flips) + 2) if aug else 0)      # 4. one per flip axis, 5. scale and shift
                drop, is_fg, u, fl, scale, shift = want
                assert m[3] == drop and m[8][0] == is_fg and m[8][1].dtype == np.uint32 and m[8][1].tolist() == u.tolist()
                assert m[8][2] == fl and m[5] == fl[0] and m[6] == scale and m[7] == shift and m[8][3] is False
                assert rec.rs.get_state()[2] == twin.get_state()[2] and (rec.rs.get_state()[1] == twin.get_state()[1]).all()
                assert all(not f for f, axis in zip(fl, 'hwd') if axis not in flips)


def test_centre_patch_draws_nothing_but_the_dropoff():
    data, store = small_store()
    ds = mrdis.VolumeDataset3D('BraTS', store, ['s0', 's1', 's2'], contrast_list=['T1', 'T2'], dropoff=True, patch_size=(2, 4, 4), patch_centre=True)
    rec = RecordingStream(3)
    metas = [ds.meta(i, rec) for i in range(3)]
    assert set(rec.calls) <= {'rand', 'choice'} and rec.calls.count('rand') == 2             # s1 has one contrast: no drop-off draw
    assert all(m[8][3] is True and not m[8][0] and m[5] is False and (m[6], m[7]) == (1.0, 0.0) for m in metas)
    assert ds.crop() == (3, 4)                                        # ((D - PD) // 2, PD)
    assert len(ds.meta(0, plain=True)) == 8                           # the windowed reads keep their meta


def test_default_path_leaves_the_global_stream_where_it_was():
    """patch_size=None: the draws of `meta` are the reference's -- drop-off, flip, scale, shift -- and nothing else"""
    data, store = small_store()
    ds = mrdis.VolumeDataset3D('BraTS', store, ['s0', 's1', 's2'], contrast_list=['T1', 'T2'], aug=True, dropoff=True)
    assert ds.patch_size is None
    np.random.seed(11)
    metas = [ds.meta(i) for i in (0, 1, 2, 0, 2)]
    after = np.random.get_state()
    np.random.seed(11)
    for i, m in zip((0, 1, 2, 0, 2), metas):
        assert len(m) == 8
        drop = -1
        if i != 1 and np.random.rand() > 0.8:
            drop = int(np.random.choice(np.array([0, 1]), 1)[0])
        flip = bool(np.random.rand() > 0.5)
        scale = 1 + 0.2 * (np.random.rand() - 0.5)
        shift = 0.2 * (np.random.rand() - 0.5)
        assert m[3:] == (drop, m[4], flip, scale, shift)
    want = np.random.get_state()
    assert after[2] == want[2] and (after[1] == want[1]).all()
    big = mrdis.VolumeStore3D.from_arrays({'s0/T1': np.zeros((2, 2, 100), np.float32)}, 'cpu')
    assert mrdis.VolumeDataset3D('BraTS', big, ['s0']).crop() == (45, 9)             # the reference's [45:-46]


def test_patch_table_words():
    data, store = small_store()
    loader = mrdis.VolumeLoader3D(mrdis.VolumeDataset3D('BraTS', store, ['s0', 's1'], contrast_list=['T1', 'T2'], aug=True), 2,
                                  patch_size=(2, 4, 4), patch_fg=0.0, patch_flips='wd')
    ds = loader.dataset
    assert ds.patch_size == (2, 4, 4) and ds.patch_flips == 'wd'
    u = np.array([1, 2, 3, 2 ** 32 - 1, 5], np.uint32)
    metas = [('s0', 0, [store.ptr('s0/T1'), store.ptr('s0/T2')], 1, store.ptr('s0/seg'), False, 1.25, -0.5, (False, u, (False, True, True), False)),
             ('s1', 0, [store.ptr('s1/T1'), 0], -1, store.ptr('s1/seg'), False, 1.0, 0.0, (False, np.zeros(5, np.uint32), (False, False, False), True))]
    tab, mask_host = loader.patch_table(metas)
    M = 2
    assert tab.shape == (2, 2 * M + patch3d.TABLE_EXTRA) and tab.dtype == np.int64 and mask_host.tolist() == [[1, 0], [1, 0]]
    assert tab[0, 0] == store.ptr('s0/T1') and tab[0, 1] == 0 and tab[0, M] == store.crop_min_ptr('s0/T1', 0, 10) and tab[0, M + 1] == 0
    assert tab[0, 2 * M] == store.ptr('s0/seg')
    assert tab[0, 2 * M + 1] == patch3d.AUG | patch3d.FLIP_W | patch3d.FLIP_D and tab[1, 2 * M + 1] == patch3d.AUG | patch3d.CENTRE
    bits = np.array([1.25, -0.5], np.float32).view(np.uint32)
    assert int(tab[0, 2 * M + 2]) & 0xffffffffffffffff == int(bits[0]) | int(bits[1]) << 32
    assert tab[0, 2 * M + 3] == 0                                    # not a foreground item: no prefix table is built or named
    assert int(tab[0, 2 * M + 4]) == 1 | 2 << 32 and int(tab[0, 2 * M + 5]) & 0xffffffffffffffff == 3 | (2 ** 32 - 1) << 32 and int(tab[0, 2 * M + 6]) == 5
    assert (patch3d.FLIP_H, patch3d.AUG, patch3d.FLIP_W, patch3d.FLIP_D, patch3d.FG, patch3d.CENTRE) == (1, 2, 4, 8, 16, 32)


def test_dataset_refusals():
    data, store = small_store()
    mk = lambda name='BraTS', **kw: mrdis.VolumeDataset3D(name, store, ['s0'], contrast_list=['T1'], **kw)
    for bad in ((2, 4), (2, 4, 0), (2.5, 4, 4), 'abc', 8, (True, 2, 2)):
        with pytest.raises(ValueError):
            mk(patch_size=bad)
    with pytest.raises(ValueError, match='does not fit'):
        mk(patch_size=(7, 8, 10))
    for bad in (-0.1, 1.5, '0.3', True):
        with pytest.raises(ValueError, match='patch_fg'):
            mk(patch_size=(2, 2, 2), patch_fg=bad)
    for bad in ('x', 'hh', None, 'hwdh'):
        with pytest.raises(ValueError, match='patch_flips'):
            mk(patch_size=(2, 2, 2), patch_flips=bad)
    with pytest.raises(ValueError, match='label targets'):
        mk('ZeroDose', patch_size=(2, 2, 2), patch_fg=0.5)
    assert mk('ZeroDose', patch_size=(2, 2, 2)).patch_fg == 0.0 and mk(patch_size=(6, 8, 10), patch_fg=1, patch_flips='').crop() == (0, 10)


# ---------------------------------------------------------------- the binding's contract (the stub-library pattern of test_hip_contracts_cpu.py)
TAB = lambda B=2, M=4, extra=0: z(B, 2 * M + patch3d.TABLE_EXTRA + extra, dtype=I64)
GEO = dict(M=4, shape=(5, 6, 7), patch=(2, 3, 4))
ROWS = {
    'fg_block_counts': (lambda: dict(seg=z(9, 11, 13), classes=(1, 2, 4)), ['fg_block_counts'], [((2, 3), I32)],
                        {'dtype': to('seg', torch.float64), 'not 3-d': put('seg', lambda: z(9, 143)), 'not dense': strided('seg'), 'no class': put('classes', lambda: ()),
                         'nine classes': put('classes', lambda: tuple(range(1, 10))), 'class 0': put('classes', lambda: (0, 1)), 'a class twice': put('classes', lambda: (1, 1)),
                         'class 256': put('classes', lambda: (256,)), 'not integers': put('classes', lambda: ('a',))}),
    'fg_prefix': (lambda: dict(seg=z(8, 16, 24), classes=(1,)), ['fg_block_counts'], [((4, 1), I32)], {'dtype': to('seg', I32), 'nine classes': put('classes', lambda: tuple(range(1, 10)))}),
    'patch_origins': (lambda: dict(table=TAB(), classes=(1, 2, 4), **GEO), ['patch_origins'], [((2, 4), I32)],
                      {'dtype': to('table', I32), 'rows short': put('table', lambda: TAB(extra=-1)), 'not dense': strided('table'), 'not 2-d': put('table', lambda: z(30, dtype=I64)),
                       'patch taller than the volume': put('patch', lambda: (6, 3, 4)), 'patch wider': put('patch', lambda: (2, 7, 4)), 'patch deeper': put('patch', lambda: (2, 3, 8)),
                       'empty patch': put('patch', lambda: (2, 0, 4)), 'a pair': put('patch', lambda: (2, 3)), 'M = 0': put('M', lambda: 0), 'M = 65': put('M', lambda: 65),
                       'nine classes': put('classes', lambda: tuple(range(1, 10))), 'class 0': put('classes', lambda: (0,)), 'no sample': put('table', lambda: TAB(B=0))}),
    'patch_gather': (lambda: dict(table=TAB(), origins=z(2, 4, dtype=I32), **GEO), ['patch_gather'], [((2, 4, 2, 3, 4), F32), ((2, 4), F32)],
                     {'table dtype': to('table', I32), 'rows short': put('table', lambda: TAB(extra=-1)), 'table not dense': strided('table'), 'origins dtype': to('origins', I64),
                      'origins short': short('origins'), 'origins narrow': put('origins', lambda: z(2, 3, dtype=I32)), 'origins not dense': strided('origins'),
                      'origins on another device': meta('origins'), 'patch larger than the volume': put('patch', lambda: (2, 3, 8)), 'K with the inputs': put('K', lambda: 3),
                      'volume of 2^31 voxels': put('shape', lambda: (2048, 1024, 1024))}),
    'patch_gather targets': (lambda: dict(table=TAB(), origins=z(2, 4, dtype=I32), targets=True, K=3, relabel=True, **GEO), ['patch_gather'], [((2, 3, 2, 3, 4), F32)],
                             {'K = 65': put('K', lambda: 65), 'K = -1': put('K', lambda: -1), 'K a float': put('K', lambda: 2.0), 'origins on another device': meta('origins')}),
    'patch_gather label': (lambda: dict(table=TAB(extra=3), origins=z(2, 4, dtype=I32), targets=True, **GEO), ['patch_gather'], [((2, 2, 3, 4), F32)],
                           {'origins long': put('origins', lambda: z(3, 4, dtype=I32))}),
}


def refusal_failures(stub):
    failures, n = [], 0
    for name, (make, _, _, mutations) in sorted(ROWS.items()):
        for what, mutate in mutations.items():
            kw = make()
            mutate(kw)
            del stub.calls[:]
            n += 1
            try:
                getattr(patch3d, name.split()[0])(**kw)
                how = 'no error'
            except hip.MrdisError:
                how = None
            except Exception as e:
                how = f'{type(e).__name__}: {e}'
            if how is not None or stub.calls:
                failures.append(f'{name} [{what}]: {how or "MrdisError"}; entry points reached: {stub.calls}')
    return failures, n


def test_every_patch_wrapper_has_a_row():
    import inspect
    wrappers = {n for n, fn in vars(patch3d).items() if inspect.isfunction(fn) and fn.__module__ == patch3d.__name__ and not n.startswith('_')}
    assert wrappers == {n.split()[0] for n in ROWS} == {'fg_block_counts', 'fg_prefix', 'patch_origins', 'patch_gather'}
    assert {'mrdis_fg_block_counts', 'mrdis_patch_origins', 'mrdis_patch_gather'} <= COMPUTE


def test_valid_calls_reach_their_entry_points(monkeypatch):
    stub = install_stub(monkeypatch.setattr)
    for name, (make, calls, shapes, _) in sorted(ROWS.items()):
        del stub.calls[:]
        result = getattr(patch3d, name.split()[0])(**make())
        assert stub.calls == calls, (name, stub.calls)
        got = [(tuple(t.shape), t.dtype) for t in tensors(result)]
        assert got == [(tuple(s), d) for s, d in shapes], (name, got)
    x, mask = patch3d.patch_gather(**ROWS['patch_gather'][0]())
    assert x.permute(0, 2, 3, 4, 1).is_contiguous()                # channels-last-3d, what model3d reads
    assert patch3d.patch_origins(table=TAB(), **GEO).shape == (2, 4)  # no classes: every sample uniform


def test_mutated_calls_raise_before_any_entry_point(monkeypatch):
    stub = install_stub(monkeypatch.setattr)
    failures, n = refusal_failures(stub)
    assert n >= 40, n
    assert not failures, '\n'.join(failures)


def test_refusals_do_not_depend_on_assert():
    """the same refusals in a child `python -O`, which strips assert statements; and the binding has no assert statement at all"""
    import ast
    tree = ast.parse(open(os.path.join(ROOT, 'representation-disentanglement_amd', 'patch3d.py')).read())
    assert not [n.lineno for n in ast.walk(tree) if isinstance(n, ast.Assert)]
    out = subprocess.run([sys.executable, '-O', os.path.abspath(__file__)], capture_output=True, text=True, timeout=300,
                         env={k: v for k, v in os.environ.items() if not k.startswith('MRDIS_')})
    assert out.returncode == 0 and 'refusals under -O: 0 failures' in out.stdout, out.stdout[-4000:] + out.stderr[-4000:]


def test_tables_match_the_header():
    txt = open(os.path.join(ROOT, 'include', 'mrdis.h')).read()
    assert int(re.search(r'#define\s+MRDIS_PATCH_MAX_CLASSES\s+(\d+)', txt).group(1)) == hip.PATCH_MAX_CLASSES == patch3d.MAX_CLASSES == 8
    assert hip.PATCH_FAMILIES == ('fgcount', 'patchorigin', 'patchgather') and set(hip.PATCH_FAMILIES) <= set(hip.launch_counts())
    assert patch3d.TABLE_EXTRA == 7 and patch3d.BLOCK == chk.BLOCK == 1024


# ---------------------------------------------------------------- config
def test_config_defaults_and_refusals():
    load = mrdis.train3d.load_config3d
    cfg = load(None, {})
    assert cfg['patch_size'] is None and cfg['patch_fg'] == 0.33 and cfg['patch_flips'] == 'hwd'
    assert load(os.path.join(ROOT, 'config3d.yaml'))['patch_size'] is None
    assert load(None, {'patch_fg': 7, 'patch_flips': 'zz'})['patch_size'] is None            # read only when patch_size is set
    cfg = load(None, {'patch_size': [128, 128, 128]})
    assert cfg['patch_size'] == [128, 128, 128]
    assert load(None, {'patch_size': (16, 32, 48), 'patch_fg': 0, 'patch_flips': ''})['patch_fg'] == 0.0
    assert load(None, {'patch_size': [8, 8, 12], 'model_name': 'UNet3D'})['patch_size'] == [8, 8, 12]
    for bad in ({'patch_size': [128, 128]}, {'patch_size': [128, 128, 100]}, {'patch_size': [16, 16, 16], 'patch_fg': 1.5},
                {'patch_size': [16, 16, 16], 'patch_flips': 'xy'}, {'patch_size': [16, 16, 0]}, {'patch_size': 16},
                {'patch_size': [16, 16, 16], 'dataset_name': 'ZeroDose'}):
        with pytest.raises(ValueError):
            load(None, bad)
    assert load(None, {'patch_size': [16, 16, 16], 'dataset_name': 'ZeroDose', 'patch_fg': 0})['patch_fg'] == 0.0


if __name__ == '__main__':
    if __debug__:
        raise SystemExit('run with python -O')
    failures, n = refusal_failures(install_stub(setattr))
    print('\n'.join(failures))
    print(f'refusals under -O: {len(failures)} failures of {n}')
    raise SystemExit(1 if failures or n < 40 else 0)
