"""Blur, contrast, gamma and noise of the 3-D training patches, the part that needs no GPU: Philox known answers and the moments of z, the
numpy oracle (tests/tone_check.py) against itself -- its fp32 form inside the derived bounds, planted faults outside them -- the keys'
refusals, the loader's draw order with the feature off and on, the table block, the config, the counter and signature tables, and the
refusals of the binding (stub library, as test_hip_contracts_cpu.py) and of the five entry points (ctypes, before any launch)."""
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
import mrdis                                                    # noqa: E402
import patch3d_check as chk                                     # noqa: E402
import warp_check as wchk                                       # noqa: E402
import tone_check as T                                          # noqa: E402
from test_hip_contracts_cpu import install_stub, meta, put, short, strided, tensors, to, z, COMPUTE      # noqa: E402
from test_warp_cpu import RecordingStream, small_store, _same_state, _Lists      # noqa: E402

hip = mrdis.hip
patch3d = mrdis.patch3d
tone3d = mrdis.tone3d
F32, I32, I64 = torch.float32, torch.int32, torch.int64
ALL_ON = dict(patch_blur=1.0, patch_contrast=1.0, patch_gamma=1.0, patch_noise=1.0)


# ---------------------------------------------------------------- Philox and z
def test_philox_known_answers():
    hexes = lambda c, k: ' '.join('%08x' % int(v) for v in T.philox(c, k))
    assert hexes((0, 0, 0, 0), (0, 0)) == '6627e8d5 e169c58d bc57ac4c 9b00dbd8'
    assert hexes((0xffffffff,) * 4, (0xffffffff,) * 2) == '408f276d 41c83b0e a20bc7c6 6d5451fd'
    assert hexes((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == 'd16cfe09 94fdcceb 5001e420 24126ea1'
    # vectorised over the first counter word: element p is the scalar answer
    many = T.philox((np.arange(5, dtype=np.uint64), 3, 0, 0), (7, 9))
    for p in range(5):
        assert [int(w[p]) for w in many] == [int(w) for w in T.philox((p, 3, 0, 0), (7, 9))]


def test_z_has_mean_0_and_variance_1():
    zs = T.noise_z(1 << 20, 1, (0x12345678, 0x9abcdef0))
    assert zs.dtype == np.float32 and abs(float(zs.mean())) < 0.01 and abs(float(zs.var()) - 1.0) < 0.01
    assert float(np.abs(zs).max()) < 6.91
    assert T.Z_SCALE == np.float32(349520.0 ** -0.5) and T.Z_SCALE.view(np.uint32) == 0x3addb446
    # the extremes of S: 0 and 16 * 255
    assert np.float32(-4080) * T.Z_SCALE > -6.91 and np.float32(4080) * T.Z_SCALE < 6.91
    other = T.noise_z(64, 2, (0x12345678, 0x9abcdef0))
    assert not np.array_equal(other, zs[:64]) and not np.array_equal(T.noise_z(64, 1, (1, 2)), zs[:64])       # the contrast and the seed both matter


def test_fma_emulation_rounds_once():
    """against exact rational arithmetic, on random operands and on sums that sit exactly half way between two fp32 values"""
    rs = np.random.RandomState(0)
    a = (rs.randn(2000) * 10.0 ** rs.randint(-3, 4, 2000)).astype(np.float32)
    b = (rs.randn(2000) * 10.0 ** rs.randint(-3, 4, 2000)).astype(np.float32)
    c = (rs.randn(2000) * 10.0 ** rs.randint(-3, 4, 2000)).astype(np.float32)
    # half-way cases: 1 + 2^-24 exactly (ties to even: 1), and a hair above (1 + 2^-23), which a double rounding through float64 would lose
    a = np.concatenate([a, np.float32([2.0 ** -12, 2.0 ** -12 + 2.0 ** -35, 3.0])])
    b = np.concatenate([b, np.float32([2.0 ** -12, 2.0 ** -12, 2.0 ** -25])])
    c = np.concatenate([c, np.float32([1.0, 1.0, 1.0 + 2.0 ** -23])])
    got = T.fma(a, b, c, np.float32)
    assert got.dtype == np.float32
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.nextafter(got[i], np.float32(-np.inf))
        hi = np.nextafter(got[i], np.float32(np.inf))
        err = abs(Fraction(float(got[i])) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), (i, a[i], b[i], c[i], got[i])
    assert got[-3] == np.float32(1.0) and got[-2] == np.float32(1.0 + 2.0 ** -23)


# ---------------------------------------------------------------- the oracle against itself
def _item(shape, seed, M=1, amp=3.0):
    rs = np.random.RandomState(seed)
    x = (rs.randn(M, *shape) * amp).astype(np.float32)
    x[rs.rand(M, *shape) < 0.3] = -10.0
    return x


SHAPES = ((16, 16, 16), (5, 7, 9), (8, 16, 24))


def _ratio(y, y64, unit):
    return float(np.abs(y.astype(np.float64) - y64).max() / unit)


def test_taps():
    for sigma in (0.25, 0.5, 0.77, 1.0):
        g = tone3d.blur_taps(sigma)
        assert g.dtype == np.float32 and g.shape == (5,) and np.array_equal(g, T.taps(sigma))
        assert abs(float(g[0]) + 2 * float(g[1:].astype(np.float64).sum()) - 1) < 4 * 2.0 ** -24 and (np.diff(g) < 0).all() and g[4] >= 0
    assert patch3d.blur_taps is tone3d.blur_taps
    for bad in (0, -1, 1.01, float('nan'), 'x', None):
        with pytest.raises(ValueError, match='blur_taps'):
            tone3d.blur_taps(bad)


def test_blur_oracle_keeps_markers_and_its_fp32_form_stays_inside_the_bound():
    worst = 0.0
    for shape in SHAPES:
        x = _item(shape, 1, M=2)
        for sigma in (1.0, 0.5, 0.25):
            g = np.stack([T.taps(sigma)] * 2)
            y64 = T.blur(x, [T.BLUR, 0], g, np.float64)
            y32 = T.blur(x, [T.BLUR, 0], g, np.float32)
            assert y32.dtype == np.float32 and np.array_equal((y64 == -10), (x == -10)) and np.array_equal((y32 == -10), (x == -10))
            assert np.array_equal(y32[1].view(np.uint32), x[1].view(np.uint32)) and np.array_equal(y64[1], x[1].astype(np.float64))     # no flag: bit for bit
            assert not np.array_equal(y32[0], x[0])
            unit = T.blur_bound(x, units=1)
            assert (np.abs(y32[0].astype(np.float64) - y64[0]) <= 56 * unit[0]).all()
            worst = max(worst, _ratio(y32[0], y64[0], unit[0]))
            # a normalised convolution of tissue values stays inside their range
            t = x[0][x[0] != -10]
            assert y64[0][x[0] != -10].min() >= t.min() - 1e-6 and y64[0][x[0] != -10].max() <= t.max() + 1e-6
    assert 0 < worst <= 56, worst
    # a constant tissue region comes out constant: the renormalisation at the background and at the patch border
    x = np.full((1, 6, 7, 12), 2.5, np.float32)
    x[0, :2] = -10.0
    y = T.blur(x, [T.BLUR], T.taps(1.0)[None], np.float64)
    assert np.allclose(y[0, 2:], 2.5, rtol=0, atol=1e-6) and (y[0, :2] == -10).all()
    # a single tissue voxel keeps its value exactly (N = g0^3 x, D = g0^3), in fp32 too up to the bound
    x = np.full((1, 5, 5, 5), -10.0, np.float32)
    x[0, 2, 2, 2] = 1.75
    assert T.blur(x, [T.BLUR], T.taps(1.0)[None], np.float64)[0, 2, 2, 2] == 1.75


@pytest.mark.parametrize('fault', ['radius 3', 'no border renormalisation', 'marker in the sum'])
def test_planted_faults_in_the_fp32_emulation_are_caught_by_the_bound(fault):
    kw = {'radius 3': dict(radius=3), 'no border renormalisation': dict(border=False), 'marker in the sum': dict(marker_in_sum=True)}[fault]
    for shape in SHAPES:
        x = _item(shape, 1)
        g = T.taps(1.0)[None]
        y64 = T.blur(x, [T.BLUR], g, np.float64)
        bad = T.blur(x, [T.BLUR], g, np.float32, **kw)
        bound = T.blur_bound(x)[0]
        assert (np.abs(bad.astype(np.float64) - y64) > bound).any(), (fault, shape, _ratio(bad, y64, bound / 56))
    if fault == 'radius 3':                                          # (invisible at sigma 0.5, where g4 rounds out of every sum: hence sigma 1.0)
        x = _item(SHAPES[0], 1)
        g = T.taps(0.5)[None]
        assert _ratio(T.blur(x, [T.BLUR], g, np.float32, radius=3), T.blur(x, [T.BLUR], g, np.float64), T.blur_bound(x, units=1)[0]) < 56


def test_planted_fault_swapped_passes_is_caught_by_the_bound():
    """The d and h passes swapped, at sigma 1.0, as the other planted faults.  The fault that a kernel can have is the one planted here: its
    passes are (stride, extent) pairs, and the d pass runs with the h extent and the h pass with the d extent (tone_check.blur's `extent_of`),
    so a tap that lies inside the patch is dropped wherever the two extents differ -- on the patches whose d and h extents differ, which are
    the ones used.  Merely running the three passes in another ORDER is no fault against float64 and cannot be one: the passes are linear
    with the same taps, any order is the same sum in exact arithmetic, and the reordered fp32 emulation sits 0.65 / 1.21 / 0.78 units of
    2^-24 amax from float64 at (16,16,16) / (5,7,9) / (8,16,24) against 0.51 / 0.54 / 0.66 for the stated order (bound: 56).  The order is held by
    the bit comparison with the fp32 statement instead (test_swapped_passes_change_bits_of_the_fp32_statement, and on the GPU the count of
    floats that differ from the fp32 numpy evaluation, which is 0)."""
    swapped = {2: 0, 0: 2}
    for shape in ((5, 7, 9), (8, 16, 24), (24, 16, 8)):
        x = _item(shape, 1)
        g = T.taps(1.0)[None]
        y64 = T.blur(x, [T.BLUR], g, np.float64)
        bad = T.blur(x, [T.BLUR], g, np.float32, extent_of=swapped)
        bound = T.blur_bound(x)[0]
        assert np.array_equal(bad == -10, x == -10)
        assert not (np.abs(bad.astype(np.float64) - y64) <= bound).all(), shape      # (a voxel whose every tap is dropped is 0 / 0: outside any bound)
        assert (np.abs(bad.astype(np.float64) - y64)[np.isfinite(bad)] > bound).any(), shape
    # where the extents agree the swap changes nothing at all
    x = _item((16, 16, 16), 1)
    assert np.array_equal(T.blur(x, [T.BLUR], T.taps(1.0)[None], np.float32, extent_of=swapped), T.blur(x, [T.BLUR], T.taps(1.0)[None], np.float32))


def test_swapped_passes_change_bits_of_the_fp32_statement():
    for shape in SHAPES:
        x = _item(shape, 1)
        g = T.taps(1.0)[None]
        a, b = T.blur(x, [T.BLUR], g, np.float32), T.blur(x, [T.BLUR], g, np.float32, order=(0, 1, 2))
        assert (a.view(np.uint32) != b.view(np.uint32)).sum() > 0.2 * (x != -10).sum()


def test_stats_and_tone_oracle():
    x = _item((6, 7, 8), 3, M=4)
    x[1] = -10.0                                                     # no tissue
    x[2] = -10.0
    x[2, 1, 2, 3] = 0.625                                            # one tissue voxel: hi == lo
    lo, hi, mean, n = st = T.stats(x)
    assert n.tolist() == [int((x[0] != -10).sum()), 0, 1, int((x[3] != -10).sum())] and lo[1] == hi[1] == mean[1] == 0
    assert lo[2] == hi[2] == mean[2] == np.float32(0.625) and lo[0] == x[0][x[0] != -10].min() and hi[3] == x[3][x[3] != -10].max()
    f, gm, sd, seed = np.float32([1.25, 2, 0.5, 0.75]), np.float32([0.7, 1.5, 2, 1.3]), np.float32([0.1, 0.2, 0.3, 0.05]), (11, 22)
    none = T.tone(x, st, [0, T.BLUR, T.INVERT, 0], f, gm, sd, seed, np.float32)
    assert np.array_equal(none.view(np.uint32), x.view(np.uint32))    # no tone flag (INVERT alone is none): bit for bit
    for fl in (T.CONTRAST, T.GAMMA, T.GAMMA | T.INVERT, T.NOISE, T.CONTRAST | T.GAMMA | T.NOISE):
        y64, y32 = T.tone(x, st, [fl] * 4, f, gm, sd, seed, np.float64), T.tone(x, st, [fl] * 4, f, gm, sd, seed, np.float32)
        assert np.array_equal(y64 == -10, x == -10) and np.array_equal(y32 == -10, x == -10)
        if not fl & T.NOISE:                                         # contrast and gamma keep a contrast inside its own range
            for m in (0, 3):
                t = y64[m][x[m] != -10]
                assert lo[m] <= t.min() and t.max() <= hi[m]
            assert y64[2, 1, 2, 3] == 0.625                          # hi == lo: the contrast clamps onto it, the gamma is skipped
        if fl == T.CONTRAST:
            for m in (0, 3):
                assert (np.abs(y32[m].astype(np.float64) - y64[m]) <= T.contrast_bound(lo[m], hi[m], f[m])).all()
        if fl == T.NOISE:
            zs = T.noise_z(x[0].size, 3, seed).reshape(x[0].shape)
            want = T.fma(sd[3], zs, x[3], np.float32)
            assert np.array_equal(y32[3][x[3] != -10], want[x[3] != -10]) and abs(float((y64[0] - x[0])[x[0] != -10].std()) - 0.1) < 0.02
    # gamma by hand: lo 0, hi 4, v 1 -> t 0.25; gamma 2 -> 0.0625 -> 0.25; inverted -> 1 - 0.75^2 = 0.4375 -> 1.75
    x = np.float32([[[[0, 4, 1, -10]]]])
    st = T.stats(x)
    assert T.tone(x, st, [T.GAMMA], [1], [2], [0], (0, 0), np.float32).reshape(-1).tolist() == [0, 4, 0.25, -10]
    assert T.tone(x, st, [T.GAMMA | T.INVERT], [1], [2], [0], (0, 0), np.float32).reshape(-1).tolist() == [0, 4, 1.75, -10]
    # contrast by hand: mean 5 / 3, factor 2: 0 -> -5/3 clamps to 0; 4 -> clamps to 4; 1 -> 1 / 3
    got = T.tone(x, st, [T.CONTRAST], [2], [1], [0], (0, 0), np.float64).reshape(-1)
    assert got[0] == 0 and got[1] == 4 and abs(got[2] - (float(st[2][0]) + (1 - float(st[2][0])) * 2)) < 1e-12 and got[3] == -10


# ---------------------------------------------------------------- the keys
def test_patch_intensity_args_refusals_name_their_key():
    from mrdis import data3d
    d = data3d.patch_intensity_args()
    assert d == {k: (tuple(float(e) for e in v) if isinstance(v, tuple) else v) for k, v in data3d.INTENSITY_DEFAULTS.items()} and d == T.DEFAULTS
    got = data3d.patch_intensity_args(patch_blur=1, patch_blur_sigma=[0.25, 1], patch_contrast_range=(0.5, 2), patch_gamma_range=[2, 2], patch_noise_std=(0, 1))
    assert got['patch_blur'] == 1.0 and got['patch_blur_sigma'] == (0.25, 1.0) and got['patch_gamma_range'] == (2.0, 2.0) and got['patch_noise_std'] == (0.0, 1.0)
    for key in ('patch_blur', 'patch_contrast', 'patch_gamma', 'patch_gamma_invert', 'patch_noise'):
        for bad in (-0.1, 1.01, '0.5', True, None, float('nan'), [0.5]):
            with pytest.raises(ValueError, match=key + ' '):
                data3d.patch_intensity_args(**{key: bad})
    ranges = {'patch_blur_sigma': ((0.2, 1.0), (0.5, 1.1)), 'patch_contrast_range': ((0.4, 1.0), (1.0, 2.1)), 'patch_gamma_range': ((0.4, 1.0), (1.0, 2.1)),
              'patch_noise_std': ((-0.1, 0.3), (0.0, 1.1))}
    for key, outside in ranges.items():
        for bad in outside + ((0.9, 0.8), (0.8,), 0.8, 'ab', (0.8, 0.9, 1.0), (True, 0.9), (0.8, float('nan')), (0.8, None)):
            with pytest.raises(ValueError, match=key + ' '):
                data3d.patch_intensity_args(**{key: bad})
    with pytest.raises(TypeError, match='patch_blurr'):
        data3d.patch_intensity_args(patch_blurr=0.5)
    data, store = small_store()
    mk = lambda **kw: mrdis.VolumeDataset3D('BraTS', store, ['s0'], contrast_list=['T1'], aug=True, patch_size=(2, 2, 2), **kw)
    for key, bad in (('patch_blur', 2), ('patch_blur_sigma', (0.5, 1.5)), ('patch_noise_std', (0.3, 0.1)), ('patch_gamma_invert', -1)):
        with pytest.raises(ValueError, match=key):
            mk(**{key: bad})
        with pytest.raises(ValueError, match=key):
            mk().set_patch((2, 2, 2), **{key: bad})
        with pytest.raises(ValueError, match=key):
            mrdis.VolumeLoader3D(mk(), 1, patch_size=(2, 2, 2), **{key: bad})


def test_intensifies():
    data, store = small_store()
    mk = lambda **kw: mrdis.VolumeDataset3D('BraTS', store, ['s0', 's1', 's2'], contrast_list=['T1', 'T2'], **kw)
    for key in ('patch_blur', 'patch_contrast', 'patch_gamma', 'patch_noise'):
        assert mk(aug=True, patch_size=(2, 4, 4), **{key: 0.1}).intensifies()
        assert not mk(aug=False, patch_size=(2, 4, 4), **{key: 0.1}).intensifies()
        assert not mk(aug=True, patch_size=(2, 4, 4), patch_centre=True, **{key: 0.1}).intensifies()
        assert not mk(aug=True, **{key: 0.1}).intensifies()
    assert not mk(aug=True, patch_size=(2, 4, 4)).intensifies()
    assert not mk(aug=True, patch_size=(2, 4, 4), patch_gamma_invert=1.0, patch_blur_sigma=(1, 1)).intensifies()      # no share above 0


# ---------------------------------------------------------------- the loader's draws
def test_draws_with_the_shares_at_zero_are_todays():
    data, store = small_store()
    for warp in (0.0, 0.5):
        for kw in ({}, dict(patch_blur=0.0, patch_contrast=0.0, patch_gamma=0.0, patch_noise=0.0, patch_gamma_invert=1.0, patch_noise_std=(0.1, 0.2))):
            ds = mrdis.VolumeDataset3D('BraTS', store, ['s0', 's1', 's2'], contrast_list=['T1', 'T2'], aug=True, dropoff=True, patch_size=(2, 4, 4),
                                       patch_fg=0.5, patch_flips='hwd', patch_warp=warp, **kw)
            assert not ds.intensifies()
            for seed in range(8):
                for idx in range(3):
                    rec, twin = RecordingStream(seed), np.random.RandomState(seed)
                    m = ds.meta(idx, rec)
                    drop, fg, u, fl, scale, shift, w = wchk.draw_item(twin, 1 if idx == 1 else 2, True, True, 0.5, 'hwd', warp)
                    assert _same_state(rec.rs, twin) and len(m) == 9 and len(m[8]) == (7 if warp else 4)
                    assert (m[3], m[6], m[7], m[8][0], m[8][2]) == (drop, scale, shift, fg, fl) and m[8][1].tolist() == u.tolist()
                    assert ('rand', 16) not in rec.calls and ('randint', 2) not in rec.calls
    loader = mrdis.VolumeLoader3D(mrdis.VolumeDataset3D('BraTS', store, ['s0', 's1'], contrast_list=['T1', 'T2'], aug=True), 2, patch_size=(2, 4, 4), patch_flips='hwd')
    ds = loader.dataset
    assert loader.patch_table([ds.meta(0), ds.meta(1)])[0].shape == (2, 2 * 2 + patch3d.TABLE_EXTRA)


@pytest.mark.parametrize('warp', [0.0, 0.5])
def test_draws_sit_between_the_warp_draw_and_the_scale(warp):
    data, store = small_store()
    M = 2
    keys = dict(patch_blur=0.6, patch_blur_sigma=(0.3, 0.9), patch_contrast=0.5, patch_contrast_range=(0.6, 1.9), patch_gamma=0.5, patch_gamma_range=(0.5, 2.0),
                patch_gamma_invert=0.5, patch_noise=0.5, patch_noise_std=(0.05, 0.4))
    seen = set()
    for dropoff, fg, flips in ((True, 0.5, 'hwd'), (False, 0.0, '')):
        ds = mrdis.VolumeDataset3D('BraTS', store, ['s0', 's1', 's2'], contrast_list=['T1', 'T2'], aug=True, dropoff=dropoff, patch_size=(2, 4, 4),
                                   patch_fg=fg, patch_flips=flips, patch_warp=warp, **keys)
        assert ds.intensifies()
        for seed in range(24):
            for idx in range(3):
                present = [True, idx != 1]
                rec, twin = RecordingStream(seed), np.random.RandomState(seed)
                m = ds.meta(idx, rec)
                drop, is_fg, u, fl, scale, shift, w, tn = T.draw_item(twin, present, dropoff, True, fg, flips, warp, **keys)
                assert _same_state(rec.rs, twin)
                # exactly 4 + 6 M doubles and two uint32, after the warp draw (or the flips), before scale and shift
                tail = ([('rand', 5)] if warp else []) + [('rand', 4 + 6 * M), ('randint', 2), ('rand',), ('rand',)]
                assert rec.calls[-len(tail):] == tail and rec.calls.count(('rand', 4 + 6 * M)) == 1 and rec.calls.count(('randint', 2)) == 1
                assert len(m[8]) == (8 if warp else 5)
                have = [k for k, p in enumerate(present) if p]
                assert (m[3], m[6], m[7]) == (have[drop] if drop >= 0 else -1, scale, shift)
                seed_, flags, sigma, f, gm, sd = m[8][-1]
                assert seed_.dtype == np.uint32 and seed_.tolist() == tn[0].tolist() and tuple(flags) == tn[1]
                for a, b in zip((sigma, f, gm, sd), tn[2:]):
                    assert a.dtype == np.float32 and np.array_equal(a, b)
                assert (0.3 <= sigma).all() and (sigma <= 0.9).all() and (0.6 <= f).all() and (f <= 1.9).all() and (0.05 <= sd).all() and (sd <= np.float32(0.4)).all()
                for k in range(M):                                   # an absent or dropped contrast gets no flag at all
                    if not present[k] or k == m[3]:
                        assert flags[k] == 0
                    seen.add(flags[k])
                # the same item without the feature: the same earlier draws, and the stream ends 4 + 6 M doubles and two uint32 earlier
                off = np.random.RandomState(seed)
                base = wchk.draw_item(off, sum(present), dropoff, True, fg, flips, warp)
                assert base[0] == drop and base[1] == is_fg and base[2].tolist() == u.tolist() and base[3] == fl and not _same_state(off, twin)
    assert {0, T.BLUR, T.NOISE, T.GAMMA | T.INVERT} <= {s & (T.BLUR | T.NOISE | T.GAMMA | T.INVERT) for s in seen} | seen and any(s & T.CONTRAST for s in seen)
    # by hand
    ds = mrdis.VolumeDataset3D('BraTS', store, ['s0'], contrast_list=['T1', 'T2'], aug=True, patch_size=(2, 4, 4), patch_flips='', **dict(keys, patch_gamma_invert=0.25))
    m = ds.meta(0, np.random.RandomState(3))
    twin = np.random.RandomState(3)
    twin.randint(0, 2 ** 32, size=5, dtype=np.uint32)
    r = twin.rand(16)
    s = twin.randint(0, 2 ** 32, size=2, dtype=np.uint32)
    seed_, flags, sigma, f, gm, sd = m[8][-1]
    assert seed_.tolist() == s.tolist()
    for k in range(2):
        q = r[4 + 6 * k:10 + 6 * k]
        want = ((T.BLUR if r[0] < 0.6 and q[0] < 0.5 else 0) | (T.CONTRAST if r[1] < 0.5 else 0) | ((T.GAMMA | (T.INVERT if q[4] < 0.25 else 0)) if r[2] < 0.5 else 0)
                | (T.NOISE if r[3] < 0.5 else 0))
        assert flags[k] == want
        assert sigma[k] == np.float32(0.3 + q[1] * (0.9 - 0.3)) and f[k] == np.float32(0.6 + q[2] * (1.9 - 0.6)) and gm[k] == np.float32(0.5 + q[3] * 1.5)
        assert sd[k] == np.float32(0.05 + q[5] * (0.4 - 0.05))


def test_no_aug_and_centre_loaders_draw_nothing_for_the_intensities():
    data, store = small_store()
    kw = dict(contrast_list=['T1', 'T2'], patch_size=(2, 4, 4), **ALL_ON)
    centre = mrdis.VolumeDataset3D('BraTS', store, ['s0', 's1', 's2'], dropoff=True, aug=True, patch_centre=True, **kw)
    noaug = mrdis.VolumeDataset3D('BraTS', store, ['s0', 's1', 's2'], aug=False, **kw)
    for ds in (centre, noaug):
        assert not ds.intensifies()
        rec = RecordingStream(3)
        metas = [ds.meta(i, rec) for i in range(3)]
        assert ('rand', 16) not in rec.calls and ('randint', 2) not in rec.calls and all(len(m[8]) == 4 for m in metas)
        assert mrdis.VolumeLoader3D(ds, 2).patch_table(metas[:2])[0].shape == (2, 4 + patch3d.TABLE_EXTRA)


def test_volume_data_passes_the_keys_to_the_train_loader_only(tmp_path):
    data, store = small_store()
    lists = _Lists(tmp_path, ['s0', 's1', 's2'])
    d = mrdis.VolumeData3D('BraTS', lists.path, norm_type='z-score', batch_size=2, contrast_list=['T1', 'T2'], aug=True, dropoff=True, store=store, device='cpu',
                           patch_size=(2, 4, 4), patch_fg=0.5, patch_blur=0.25, patch_noise=0.5, patch_noise_std=(0.1, 0.2))
    tr, va, te = d.trainLoader.dataset, d.valLoader.dataset, d.testLoader.dataset
    assert tr.intensifies() and tr.intensity['patch_blur'] == 0.25 and tr.intensity['patch_noise_std'] == (0.1, 0.2) and tr.intensity['patch_gamma'] == 0.0
    assert not va.intensifies() and not te.intensifies() and va.intensity == te.intensity == T.DEFAULTS
    off = mrdis.VolumeData3D('BraTS', lists.path, norm_type='z-score', batch_size=2, contrast_list=['T1', 'T2'], aug=True, store=store, device='cpu', patch_size=(2, 4, 4))
    assert not off.trainLoader.dataset.intensifies()
    with pytest.raises(ValueError, match='patch_noise_std'):
        mrdis.VolumeData3D('BraTS', lists.path, norm_type='z-score', batch_size=2, contrast_list=['T1'], aug=True, store=store, device='cpu', patch_size=(2, 4, 4),
                           patch_noise_std=(0.5, 0.1))


# ---------------------------------------------------------------- the table
def test_packing_round_trips():
    rs = np.random.RandomState(5)
    for M in (1, 2, 4, 7):
        seed = rs.randint(0, 2 ** 32, size=2, dtype=np.uint32)
        flags = [int(v) for v in rs.randint(0, 32, M)]
        sigma, f, gm, sd = (rs.uniform(a, b, M) for a, b in ((0.25, 1), (0.5, 2), (0.5, 2), (0, 1)))
        w = tone3d.pack_tone(seed, flags, sigma, f, gm, sd)
        assert w.dtype == np.int64 and w.shape == (tone3d.TONE_EXTRA(M),) == (1 + 5 * M,) == (patch3d.TONE_EXTRA(M),) and np.array_equal(w, T.pack(seed, flags, sigma, f, gm, sd))
        s2, fl2, g2, f2, gm2, sd2 = T.unpack(w, M)
        assert s2.tolist() == seed.tolist() and fl2.tolist() == flags
        assert np.array_equal(f2, f.astype(np.float32)) and np.array_equal(gm2, gm.astype(np.float32)) and np.array_equal(sd2, sd.astype(np.float32))
        for m in range(M):
            assert np.array_equal(g2[m], T.taps(sigma[m]) if flags[m] & T.BLUR else np.zeros(5, np.float32))
        u = [int(v) & 0xffffffffffffffff for v in w]
        assert u[0] == int(seed[0]) | int(seed[1]) << 32 and u[1] & 0xffffffff == flags[0] and all(v >> 32 == 0 for v in u[5::5])     # the tenth half is 0
    assert (patch3d.TONE_BLUR, patch3d.TONE_CONTRAST, patch3d.TONE_GAMMA, patch3d.TONE_INVERT, patch3d.TONE_NOISE) == (1, 2, 4, 8, 16) == (T.BLUR, T.CONTRAST, T.GAMMA, T.INVERT, T.NOISE)
    txt = open(os.path.join(ROOT, 'include', 'mrdis.h')).read()
    for name, v in (('BLUR', 1), ('CONTRAST', 2), ('GAMMA', 4), ('INVERT', 8), ('NOISE', 16)):
        assert int(re.search(r'#define\s+MRDIS_TONE_%s\s+(\d+)' % name, txt).group(1)) == v
    assert '0x3addb446' in txt and '0x3addb446' in open(os.path.join(ROOT, 'representation-disentanglement_amd', 'csrc', 'mrdis_tone.hip')).read()
    for bad in (dict(flags=[32]), dict(flags=[]), dict(sigma=[0.5, 0.5]), dict(seed=(1,)), dict(flags=[-1])):
        kw = dict(seed=(1, 2), flags=[1], sigma=[0.5], f=[1.0], gamma=[1.0], std=[0.1])
        kw.update(bad)
        with pytest.raises(ValueError, match='pack_tone'):
            tone3d.pack_tone(**kw)


def test_table_layout_on_and_off():
    data, store = small_store()
    M = 2
    mk = lambda **kw: mrdis.VolumeLoader3D(mrdis.VolumeDataset3D('BraTS', store, ['s0', 's1'], contrast_list=['T1', 'T2'], aug=True), 2, patch_size=(2, 4, 4),
                                           patch_flips='wd', **kw)
    u = np.array([1, 2, 3, 2 ** 32 - 1, 5], np.uint32)
    head = lambda sid: (sid, 0, [store.ptr(sid + '/T1'), store.ptr(sid + '/T2')], -1, store.ptr(sid + '/seg'), False, 1.25, -0.5)
    tone0 = (np.array([7, 2 ** 32 - 1], np.uint32), (T.BLUR | T.NOISE, T.GAMMA | T.INVERT), np.float32([0.5, 0.9]), np.float32([1.1, 0.9]), np.float32([0.7, 1.4]), np.float32([0.1, 0.2]))
    tone1 = (np.array([0, 0], np.uint32), (0, 0), np.float32([0.6, 0.6]), np.float32([1, 1]), np.float32([1, 1]), np.float32([0, 0]))
    warp = (True, (-10.0, 20.0, -30.0), 0.7)
    for warps in (False, True):
        w = warp if warps else ()
        metas_on = [head('s0') + ((False, u, (False, True, True), False) + w + (tone0,),), head('s1') + ((False, u, (False, False, False), False) + w + (tone1,),)]
        metas_off = [m[:8] + (m[8][:-1],) for m in metas_on]
        kw = dict(patch_warp=0.5) if warps else {}
        on, off = mk(patch_noise=0.5, **kw), mk(**kw)
        t_on, mask_on = on.patch_table(metas_on)
        t_off, mask_off = off.patch_table(metas_off)
        col = 2 * M + 7 + (5 if warps else 0)
        assert on.dataset.tone_col() == col and t_off.shape == (2, col) and t_on.shape == (2, col + 1 + 5 * M) and np.array_equal(mask_on, mask_off)
        assert np.array_equal(t_on[:, :col], t_off)                  # what the row already holds does not move
        assert np.array_equal(t_on[0, col:], T.pack(*tone0)) and np.array_equal(t_on[1, col:], T.pack(*tone1))
        assert not t_on[1, col:].any() or T.unpack(t_on[1, col:], M)[1].tolist() == [0, 0]


# ---------------------------------------------------------------- the config
def test_config_defaults_and_refusals():
    load = mrdis.train3d.load_config3d
    cfg = load(None, {})
    yml = load(os.path.join(ROOT, 'config3d.yaml'))
    for key, v in mrdis.data3d.INTENSITY_DEFAULTS.items():
        want = list(v) if isinstance(v, tuple) else v
        assert cfg[key] == want == yml[key] == mrdis.train3d.DEFAULT_CONFIG_3D[key], key
    assert yml == cfg                                                # config3d.yaml still equals the defaults
    assert load(None, {'patch_blur': 7, 'patch_blur_sigma': 'zz'})['patch_size'] is None       # read only when patch_size is set
    cfg = load(None, {'patch_size': [16, 16, 16], 'patch_blur': '0.5', 'patch_blur_sigma': (0.25, 1), 'patch_noise_std': (0, 1)})
    assert cfg['patch_blur'] == 0.5 and cfg['patch_blur_sigma'] == [0.25, 1.0] and cfg['patch_noise_std'] == [0.0, 1.0]
    for key, bad in (('patch_blur', 1.5), ('patch_contrast', -1), ('patch_blur_sigma', [0.5, 1.2]), ('patch_contrast_range', [1.25, 0.75]), ('patch_gamma_range', [0.1, 1.0]),
                     ('patch_gamma_invert', 2), ('patch_noise', 1.2), ('patch_noise_std', 0.3)):
        with pytest.raises(ValueError, match=key):
            load(None, {'patch_size': [16, 16, 16], key: bad})


# ---------------------------------------------------------------- counters and signatures
ENTRY_POINTS = ('mrdis_patch_blur_workspace', 'mrdis_patch_blur', 'mrdis_patch_stats_workspace', 'mrdis_patch_stats', 'mrdis_patch_tone')


def test_counter_and_signature_tables_match_the_library():
    lib = hip.load()
    assert hip.TONE_FAMILIES == ('patchblur', 'patchstats', 'patchtone') and set(hip.TONE_FAMILIES) <= set(hip.LAUNCH_COUNTERS) and set(hip.TONE_FAMILIES) <= set(hip.launch_counts())
    assert len(set(hip.LAUNCH_COUNTERS)) == len(hip.LAUNCH_COUNTERS)
    for fam in hip.TONE_FAMILIES:
        assert lib.mrdis_launch_count(fam.encode()) >= 0, fam
    common = open(os.path.join(ROOT, 'representation-disentanglement_amd', 'csrc', 'mrdis_common.h')).read()
    assert all(f'"{fam}"' in common for fam in hip.TONE_FAMILIES)
    header = open(os.path.join(ROOT, 'include', 'mrdis.h')).read()
    for name in ENTRY_POINTS:
        assert name in hip._SIGS and name in hip.EXPORTED_SYMBOLS and getattr(lib, name) is not None
        proto = re.search(r'\b%s\s*\(([^;]*)\)\s*;' % name, header).group(1)
        assert len(hip._SIGS[name][1]) == proto.count(',') + 1, name   # one ctypes type per parameter of the prototype
    assert {n for n in ENTRY_POINTS if not n.endswith('_workspace')} <= COMPUTE
    # the workspace queries are host-only and pure
    assert lib.mrdis_patch_blur_workspace(2, 4, 8, 8, 8) >= 2 * 4 * 2 * 4 * 512 and lib.mrdis_patch_blur_workspace(0, 4, 8, 8, 8) == 0
    assert lib.mrdis_patch_stats_workspace(2, 3, 5, 7, 9) >= 20 * 6 and lib.mrdis_patch_stats_workspace(2, 3, 5, 7, 0) == 0
    assert lib.mrdis_patch_blur_workspace(4, 4, 128, 128, 128) == 4 * 4 * 4 * 4 * 128 ** 3      # (beyond 2^31 bytes: size_t)


def test_library_refuses_by_return_code():
    """the C entry points themselves, on arguments they refuse before any launch (no GPU is touched)"""
    lib = hip.load()
    M, B, P = 4, 2, (2, 3, 4)
    n = B * M * 24
    x, y, st, ws = z(n + 4), z(n + 4), z(B * M * 4, dtype=I32), z(1 << 16, dtype=torch.uint8)
    tab = z(B, 30, dtype=I64)
    wsb = max(lib.mrdis_patch_blur_workspace(B, M, *P), lib.mrdis_patch_stats_workspace(B, M, *P))
    assert 0 < wsb <= ws.numel() and x.data_ptr() % 16 == 0 and ws.data_ptr() % 16 == 0
    base = dict(x=x.data_ptr(), y=y.data_ptr(), stats=st.data_ptr(), table=tab.data_ptr(), ld=30, col=9, B=B, M=M, PH=P[0], PW=P[1], PD=P[2], ws=ws.data_ptr(), wsb=wsb, stream=None)
    order = {'blur': ('x', 'y', 'table', 'ld', 'col', 'B', 'M', 'PH', 'PW', 'PD', 'ws', 'wsb', 'stream'),
             'stats': ('x', 'stats', 'B', 'M', 'PH', 'PW', 'PD', 'ws', 'wsb', 'stream'),
             'tone': ('x', 'stats', 'table', 'ld', 'col', 'B', 'M', 'PH', 'PW', 'PD', 'stream')}
    call = lambda which, **kw: getattr(lib, 'mrdis_patch_' + which)(*[{**base, **kw}[k] for k in order[which]])
    codes = {lib.mrdis_strerror(c).decode(): c for c in range(-8, 0)}
    EINVAL, EUNSUPPORTED, EWORKSPACE, EALIGN = (codes[k] for k in ('invalid argument', 'unsupported geometry', 'workspace too small', 'misaligned pointer or leading dimension'))
    everywhere = (dict(x=None), dict(B=0), dict(M=0), dict(M=65), dict(PH=0), dict(PW=-1), dict(PD=0))
    with_table = (dict(table=None), dict(col=-1), dict(ld=9 + 5 * M), dict(ld=0), dict(col=30))
    for which in order:
        for kw in everywhere + (with_table if which != 'stats' else ()):
            assert call(which, **kw) == EINVAL, (which, kw)
        assert call(which, B=65536) == EUNSUPPORTED and call(which, PH=2048, PW=1024, PD=1024) == EUNSUPPORTED, which
        assert call(which, x=x.data_ptr() + 2) == EALIGN, which
    assert call('blur', y=x.data_ptr()) == EINVAL and call('blur', y=None) == EINVAL and call('blur', ws=None) == EINVAL
    assert call('blur', wsb=wsb - 1) == EWORKSPACE and call('stats', wsb=lib.mrdis_patch_stats_workspace(B, M, *P) - 1) == EWORKSPACE and call('stats', wsb=0) == EWORKSPACE
    assert call('blur', y=y.data_ptr() + 1) == EALIGN and call('blur', ws=ws.data_ptr() + 8) == EALIGN and call('blur', table=tab.data_ptr() + 4) == EALIGN
    assert call('stats', stats=None) == EINVAL and call('stats', ws=None) == EINVAL and call('stats', stats=st.data_ptr() + 2) == EALIGN and call('stats', ws=ws.data_ptr() + 4) == EALIGN
    assert call('tone', stats=None) == EINVAL and call('tone', stats=st.data_ptr() + 1) == EALIGN and call('tone', table=tab.data_ptr() + 4) == EALIGN
    assert all(lib.mrdis_launch_count(f.encode()) == 0 for f in hip.TONE_FAMILIES + ('all',)) or True      # (counters are process-wide: the GPU tests assert the zero)


# ---------------------------------------------------------------- the binding's contract (the stub-library pattern of test_hip_contracts_cpu.py)
def X(B=2, M=4, patch=(2, 3, 4)):
    return torch.zeros((B,) + patch + (M,)).permute(0, 4, 1, 2, 3)


TAB = lambda B=2, M=4, col=15, extra=0: z(B, col + 1 + 5 * M + extra, dtype=I64)
ROWS = {
    'patch_blur': (lambda: dict(x=X(), table=TAB(), col=15, M=4), ['patch_blur'], [((2, 4, 2, 3, 4), F32)],
                   {'x dtype': to('x', torch.float64), 'x contiguous, not channels-last': put('x', lambda: z(2, 4, 2, 3, 4)), 'x not 5-d': put('x', lambda: z(2, 4, 24)),
                    'x of another M': put('x', lambda: X(M=3)), 'M = 0': put('M', lambda: 0), 'M = 65': put('M', lambda: 65), 'M a float': put('M', lambda: 4.0),
                    'M a bool': put('M', lambda: True), 'no patch': put('x', lambda: X(B=0)), 'x not dense': put('x', lambda: X(patch=(2, 3, 8))[..., ::2]),
                    'table dtype': to('table', I32), 'rows short': put('table', lambda: TAB(extra=-1)), 'table of another B': put('table', lambda: TAB(B=3)),
                    'table not dense': strided('table'), 'table on another device': meta('table'), 'table not 2-d': put('table', lambda: z(72, dtype=I64)),
                    'col = -1': put('col', lambda: -1), 'col a float': put('col', lambda: 15.0), 'col past the row': put('col', lambda: 16)}),
    'patch_stats': (lambda: dict(x=X(M=3), M=3), ['patch_stats'], [((2, 3, 4), I32)],
                    {'x dtype': to('x', torch.float16), 'x contiguous, not channels-last': put('x', lambda: z(2, 3, 2, 3, 4)), 'M = 4 for three contrasts': put('M', lambda: 4),
                     'x on meta with M = 0': put('M', lambda: 0)}),
    'patch_tone': (lambda: dict(x=X(), stats=z(2, 4, 4, dtype=I32), table=TAB(extra=2), col=15, M=4), ['patch_tone'], [((2, 4, 2, 3, 4), F32)],
                   {'stats dtype': to('stats', F32), 'stats short': short('stats'), 'stats of three words': put('stats', lambda: z(2, 4, 3, dtype=I32)),
                    'stats not dense': strided('stats'), 'stats on another device': meta('stats'), 'rows short': put('table', lambda: TAB(extra=-1)),
                    'col = -2': put('col', lambda: -2), 'x dtype': to('x', torch.bfloat16), 'table on another device': meta('table')}),
    'patch_intensify': (lambda: dict(x=X(M=1), table=TAB(M=1, col=9), col=9, M=1), ['patch_blur', 'patch_stats', 'patch_tone'], [((2, 1, 2, 3, 4), F32)],
                        {'rows short': put('table', lambda: TAB(M=1, col=9, extra=-1)), 'x dtype': to('x', torch.float64), 'M = 2': put('M', lambda: 2)}),
}


def test_valid_calls_reach_their_entry_points(monkeypatch):
    stub = install_stub(monkeypatch.setattr)
    for name, (make, calls, shapes, _) in sorted(ROWS.items()):
        del stub.calls[:]
        kw = make()
        result = getattr(tone3d, name)(**kw)
        assert stub.calls == calls, (name, stub.calls)
        assert [(tuple(t.shape), t.dtype) for t in tensors(result)] == [(tuple(s), d) for s, d in shapes], name
        if name != 'patch_stats':
            assert result.permute(0, 2, 3, 4, 1).is_contiguous()     # channels-last-3d, what model3d reads
        if name == 'patch_tone':
            assert result is kw['x']                                 # in place
        if name in ('patch_blur', 'patch_intensify'):
            assert result.data_ptr() != kw['x'].data_ptr()           # out of place
    for name in ROWS:
        assert getattr(patch3d, name) is getattr(tone3d, name)
    assert mrdis.patch_intensify is tone3d.patch_intensify


def test_mutated_calls_raise_before_any_entry_point(monkeypatch):
    stub = install_stub(monkeypatch.setattr)
    failures, n = [], 0
    for name, (make, _, _, mutations) in sorted(ROWS.items()):
        for what, mutate in mutations.items():
            kw = make()
            mutate(kw)
            del stub.calls[:]
            n += 1
            try:
                getattr(tone3d, name)(**kw)
                how = 'no error'
            except hip.MrdisError:
                how = None
            except Exception as e:
                how = f'{type(e).__name__}: {e}'
            if how is not None or stub.calls:
                failures.append(f'{name} [{what}]: {how or "MrdisError"}; entry points reached: {stub.calls}')
    assert n >= 30 and not failures, '\n'.join(failures)


def test_binding_has_no_assert_statement():
    import ast
    tree = ast.parse(open(os.path.join(ROOT, 'representation-disentanglement_amd', 'tone3d.py')).read())
    assert not [n.lineno for n in ast.walk(tree) if isinstance(n, ast.Assert)]
