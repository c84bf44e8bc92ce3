"""Blur, contrast, gamma and noise of the 3-D training patches on the GPU (csrc/mrdis_tone.hip, tone3d.py, data3d.py's intensity keys, Run3D)
against the plain-numpy oracle tests/tone_check.py.  Tensors are built directly, without a store.
Exact: the -10 markers, every row and contrast without a flag, lo / hi / n of the statistics, the noise term (fmaf(std, z, v) against the
oracle's exact fused multiply-add), run against run, the M = 4 kernels against the generic ones (debug_volgen, and a base that is only 4-byte
aligned), every flag at once against the three steps one after the other.
Bounded: the blur within 56 * 2^-24 amax of float64 (tone_check.blur_bound), the contrast within (4 |f| + 2) * 2^-24 max(|lo|, |hi|)
(tone_check.contrast_bound), the mean within one fp32 ulp, the gamma within kappa * 2^-24 max(|lo|, |hi|), kappa = 4 times the worst ratio of
the plain fp32 numpy evaluation of the same rows (numpy.power in fp32) to float64, at least 4: powf is a library function (tests/aux_check.py's
practice).  The kernels' worst ratios and the yardsticks per case: profiles/tone_path_margins.txt, recorded with MRDIS_DUMP_MEASURED=<dir>."""
import math

import numpy as np
import pytest
import torch

import patch3d_check as chk
import tone_check as T
from fixtures import dump_measured
from fixtures_data3d import data3d_volumes, data3d_subjects

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
ALL = T.BLUR | T.CONTRAST | T.GAMMA | T.NOISE

# name -> (M, patch)
CASES = {
    'm4 cube': (4, (16, 16, 16)),
    'm4 slab': (4, (8, 16, 24)),                   # partial tiles along w and d
    'm2 cube': (2, (16, 16, 16)),                  # generic
    'm3 odd': (3, (5, 7, 9)),                      # generic; 5 and 7 lie below the 9 taps: both borders fall in one window
    'm4 column': (4, (1, 1, 40)),                  # a single column: the w and h passes see one voxel
    'm1 long': (1, (4, 4, 72)),
}
_REF = {}


def to_dev(x):
    """(B, M, PH, PW, PD) numpy -> the layout the gathers return: a permuted view of a dense (B, PH, PW, PD, M) tensor"""
    return torch.from_numpy(np.ascontiguousarray(np.moveaxis(x, 1, -1))).to(DEV).permute(0, 4, 1, 2, 3)


def to_host(t):
    return t.detach().cpu().numpy()


def _case(name):
    """the six rows of a case, their table blocks and the float64 / fp32 blur of the oracle, built once"""
    if name in _REF:
        return _REF[name]
    M, patch = CASES[name]
    seed = sorted(CASES).index(name)
    rs = np.random.RandomState(200 + seed)
    B = 6
    x = (rs.randn(B, M, *patch) * (1.0 + seed)).astype(np.float32)
    x[rs.rand(B, M, *patch) < 0.3] = -10.0
    x[4, 0] = -10.0                                                  # an all-background contrast
    if M > 1:
        x[4, 1] = 0.0                                                # an absent contrast: zeros, which are tissue and carry no flag
    x[5, 0] = -10.0
    x[5, 0][tuple(p // 2 for p in patch)] = 0.875                    # a single tissue voxel: hi == lo
    two = [T.BLUR if m < 2 else 0 for m in range(M)]
    absent = [0 if (m == 1 and M > 1) else ALL for m in range(M)]
    flags = [[ALL] * M, [ALL | T.INVERT] * M, two, [0] * M, absent, [ALL] * M]
    sigma = [[1.0] * M, [0.5] * M, [0.8] * M, [0.7] * M, [1.0] * M, [0.6] * M]
    rows = []
    for b in range(B):
        rows.append(dict(seed=rs.randint(0, 2 ** 32, size=2, dtype=np.uint32), flags=flags[b], sigma=np.float32(sigma[b]),
                         f=rs.uniform(0.5, 2.0, M).astype(np.float32), gamma=rs.uniform(0.5, 2.0, M).astype(np.float32), std=rs.uniform(0.05, 0.3, M).astype(np.float32)))
    blocks = np.stack([T.pack(r['seed'], r['flags'], r['sigma'], r['f'], r['gamma'], r['std']) for r in rows])
    halves = blocks.view(np.uint32).copy()                           # row 3: junk in every value field, flags 0
    junk = rs.randint(0, 2 ** 32, size=halves.shape[1], dtype=np.uint32)
    junk[2::10][:M] = 0
    halves[3] = junk
    halves[3, 2 + np.arange(M) * 10 + 1] = 0x7fc00000               # (a NaN tap among them)
    blocks = halves.view(np.int64)
    g = np.stack([np.stack([T.taps(s) for s in r['sigma']]) for r in rows])
    y64 = np.stack([T.blur(x[b], rows[b]['flags'], g[b], np.float64) for b in range(B)])
    y32 = np.stack([T.blur(x[b], rows[b]['flags'], g[b], np.float32) for b in range(B)])
    _REF[name] = dict(x=x, rows=rows, blocks=blocks, y64=y64, y32=y32, unit=np.stack([T.blur_bound(x[b], units=1) for b in range(B)]))
    return _REF[name]


def _table(M, blocks, rs=None):
    """rows of 2 M + 7 words the three calls never read (junk), then the block"""
    col = 2 * M + 7
    head = (rs or np.random.RandomState(1)).randint(-2 ** 62, 2 ** 62, size=(len(blocks), col), dtype=np.int64)
    return torch.from_numpy(np.concatenate([head, blocks], axis=1)).to(DEV), col


def _with_flags(ref, M, keep):
    """the case's table with every flag word masked by `keep`"""
    halves = ref['blocks'].view(np.uint32).copy()
    for m in range(M):
        halves[:, 2 + 10 * m] &= keep
    return _table(M, halves.view(np.int64))


def _counts(hip, **want):
    c = hip.launch_counts()
    for k, v in want.items():
        assert c[k] == v, (k, c[k], v)
    assert sum(v for k, v in c.items() if k not in want) == 0, {k: v for k, v in c.items() if v and k not in want}


@pytest.mark.parametrize('name', sorted(CASES))
def test_blur_and_stats_against_the_oracle(mrdis, name):
    hip, p = mrdis.hip, mrdis.patch3d
    M, patch = CASES[name]
    ref = _case(name)
    x = to_dev(ref['x'])
    tab, col = _table(M, ref['blocks'])
    assert tab.shape[1] == col + p.TONE_EXTRA(M)
    vec = M == 4
    hip.launch_counts(reset=True)
    y = p.patch_blur(x, tab, col, M)
    _counts(hip, patchblur=1, all=2 if vec else 3)
    assert y.shape == x.shape and y.stride() == x.stride() and y.data_ptr() != x.data_ptr()
    assert torch.equal(x, to_dev(ref['x']))                         # out of place: x is left as it was
    # run against run; the M = 4 kernels against the generic ones, by the switch and by a base that is only 4-byte aligned
    assert torch.equal(p.patch_blur(x, tab, col, M).view(torch.int32), y.view(torch.int32))
    if vec:
        hip.set_option('debug_volgen', 1)
        hip.launch_counts(reset=True)
        yg = p.patch_blur(x, tab, col, M)
        _counts(hip, patchblur=1, all=3)
        hip.set_option('debug_volgen', 0)
        assert torch.equal(yg.view(torch.int32), y.view(torch.int32))
        buf = torch.empty(x.numel() + 1, device=DEV)
        xo = buf[1:].view(x.shape[0], *patch, M).permute(0, 4, 1, 2, 3)
        xo.copy_(x)
        assert xo.data_ptr() % 16 == 4
        hip.launch_counts(reset=True)
        yo = p.patch_blur(xo, tab, col, M)
        _counts(hip, patchblur=1, all=3)
        assert torch.equal(yo.view(torch.int32), y.view(torch.int32))
    yn, xn = to_host(y), ref['x']
    np.testing.assert_array_equal(yn == -10, xn == -10, err_msg=f'{name}: the -10 markers')
    assert np.isfinite(yn).all()
    failures = []
    for b, row in enumerate(ref['rows']):
        for m in range(M):
            if not row['flags'][m] & T.BLUR or b == 3:
                assert np.array_equal(yn[b, m].view(np.uint32), xn[b, m].view(np.uint32)), (name, b, m)      # bit for bit
                continue
            unit = ref['unit'][b, m]
            err = np.abs(yn[b, m].astype(np.float64) - ref['y64'][b, m])
            ratio = float(err.max() / unit) if unit > 0 else float(err.max())
            yard = float(np.abs(ref['y32'][b, m].astype(np.float64) - ref['y64'][b, m]).max() / unit) if unit > 0 else 0.0
            bits = int((yn[b, m].view(np.uint32) != ref['y32'][b, m].view(np.uint32)).sum())
            print(f'{name} row {b} contrast {m}: blur kernel {ratio:.3f} units, fp32 numpy {yard:.3f} units, {bits} of {yn[b, m].size} floats differ from fp32 numpy')
            dump_measured('tone_path_margins.jsonl', dict(step='blur', case=name, row=b, contrast=m, M=M, patch=patch, sigma=float(row['sigma'][m]), bound=56, kernel=ratio,
                                                          yardstick=yard, differ_from_fp32_numpy=bits, floats=int(yn[b, m].size)))
            if not (err <= 56 * unit).all():
                failures.append(f'{name} row {b} contrast {m}: {ratio:.2f} units > 56 (fp32 numpy: {yard:.2f})')
    assert not failures, '\n'.join(failures)
    # statistics of the kernel's own y
    hip.launch_counts(reset=True)
    st = p.patch_stats(y, M)
    _counts(hip, patchstats=1, all=2)
    assert st.shape == (len(yn), M, 4) and st.dtype == torch.int32 and torch.equal(st, p.patch_stats(y, M))
    if vec:
        hip.set_option('debug_volgen', 1)
        sg = p.patch_stats(y, M)
        hip.set_option('debug_volgen', 0)
        assert torch.equal(sg, st)
    sn = to_host(st)
    for b in range(len(yn)):
        lo, hi, mean, n = T.stats(yn[b])
        assert sn[b, :, 3].tolist() == n.tolist() and np.array_equal(sn[b, :, 0].view(np.float32), lo) and np.array_equal(sn[b, :, 1].view(np.float32), hi), (name, b)
        got = np.ascontiguousarray(sn[b, :, 2]).view(np.float32)
        for m in range(M):
            assert got[m] == mean[m] or got[m] in (np.nextafter(mean[m], np.float32(np.inf)), np.nextafter(mean[m], np.float32(-np.inf))), (name, b, m, got[m], mean[m])
    assert sn[4, 0].tolist() == [0, 0, 0, 0] and sn[5, 0, 3] == 1 and sn[5, 0, 0] == sn[5, 0, 1] == sn[5, 0, 2]      # no tissue; a single tissue voxel


def _stats_of(sn, b):
    f32 = lambda k: np.ascontiguousarray(sn[b, :, k]).view(np.float32)
    return f32(0), f32(1), f32(2), sn[b, :, 3]


@pytest.mark.parametrize('name', sorted(CASES))
def test_tone_against_the_oracle(mrdis, name):
    hip, p = mrdis.hip, mrdis.patch3d
    M, patch = CASES[name]
    ref = _case(name)
    tab, col = _table(M, ref['blocks'])
    y = p.patch_blur(to_dev(ref['x']), tab, col, M)
    st = p.patch_stats(y, M)
    yn, sn = to_host(y), to_host(st)
    B = len(yn)

    def run(keep, src=y, form=0):
        t, _ = _with_flags(ref, M, keep)
        v = src.clone()
        assert v.stride() == src.stride()
        hip.set_option('debug_volgen', form)
        hip.launch_counts(reset=True)
        out = p.patch_tone(v, st, t, col, M)
        _counts(hip, patchtone=1, all=1)
        hip.set_option('debug_volgen', 0)
        assert out is v
        return v

    params = lambda b: (ref['rows'][b]['f'], ref['rows'][b]['gamma'], ref['rows'][b]['std'], ref['rows'][b]['seed'])
    live = [b for b in range(B) if b != 3]
    fl = lambda b, keep: [f & keep for f in ref['rows'][b]['flags']]
    # no tone flag at all (the blur flag alone): bit for bit
    assert torch.equal(run(T.BLUR | T.INVERT).view(torch.int32), y.view(torch.int32))
    # noise alone: fmaf(std, z, v), bit-equal to the oracle
    vn = to_host(run(T.NOISE))
    for b in range(B):
        want = T.tone(yn[b], _stats_of(sn, b), fl(b, T.NOISE) if b != 3 else [0] * M, *params(b), np.float32)
        assert np.array_equal(vn[b].view(np.uint32), want.view(np.uint32)), (name, b)
    assert not np.array_equal(vn[0], yn[0])
    # contrast alone: the derived bound against float64
    vc = to_host(run(T.CONTRAST))
    failures = []
    for b in live:
        lo, hi, mean, n = _stats_of(sn, b)
        want = T.tone(yn[b], (lo, hi, mean, n), fl(b, T.CONTRAST), *params(b), np.float64)
        yard32 = T.tone(yn[b], (lo, hi, mean, n), fl(b, T.CONTRAST), *params(b), np.float32)
        for m in range(M):
            if not ref['rows'][b]['flags'][m] & T.CONTRAST:
                assert np.array_equal(vc[b, m].view(np.uint32), yn[b, m].view(np.uint32))
                continue
            f = float(ref['rows'][b]['f'][m])
            unit = T.contrast_bound(lo[m], hi[m], f, units=1)
            err = np.abs(vc[b, m].astype(np.float64) - want[m])
            ratio = float(err.max() / unit) if unit > 0 else float(err.max())
            yard = float(np.abs(yard32[m].astype(np.float64) - want[m]).max() / unit) if unit > 0 else 0.0
            print(f'{name} row {b} contrast {m}: contrast kernel {ratio:.3f} units, fp32 numpy {yard:.3f}, bound {4 * f + 2:.2f}')
            dump_measured('tone_path_margins.jsonl', dict(step='contrast', case=name, row=b, contrast=m, M=M, patch=patch, f=f, bound=4 * f + 2, kernel=ratio, yardstick=yard))
            if not (err <= T.contrast_bound(lo[m], hi[m], f)).all():
                failures.append(f'{name} row {b} contrast {m}: contrast {ratio:.2f} units > {4 * f + 2:.2f}')
            t = vc[b, m][yn[b, m] != -10]
            assert t.size == 0 or (lo[m] <= t.min() and t.max() <= hi[m])
    # gamma alone (rows 1: the inverted curve): kappa
    vg = to_host(run(T.GAMMA | T.INVERT))
    for b in live:
        lo, hi, mean, n = _stats_of(sn, b)
        want = T.tone(yn[b], (lo, hi, mean, n), fl(b, T.GAMMA | T.INVERT), *params(b), np.float64)
        yard32 = T.tone(yn[b], (lo, hi, mean, n), fl(b, T.GAMMA | T.INVERT), *params(b), np.float32)
        for m in range(M):
            if not ref['rows'][b]['flags'][m] & T.GAMMA or not hi[m] > lo[m]:
                assert np.array_equal(vg[b, m].view(np.uint32), yn[b, m].view(np.uint32)), (name, b, m)      # no flag, or hi == lo: skipped
                continue
            unit = T.gamma_unit(lo[m], hi[m])
            err = np.abs(vg[b, m].astype(np.float64) - want[m])
            ratio, yard = float(err.max() / unit), float(np.abs(yard32[m].astype(np.float64) - want[m]).max() / unit)
            kappa = max(4, math.ceil(4 * yard))
            print(f'{name} row {b} contrast {m}: gamma kernel {ratio:.3f} units, fp32 numpy {yard:.3f}, kappa {kappa}')
            dump_measured('tone_path_margins.jsonl', dict(step='gamma', case=name, row=b, contrast=m, M=M, patch=patch, gamma=float(ref['rows'][b]['gamma'][m]),
                                                          inverted=bool(ref['rows'][b]['flags'][m] & T.INVERT), bound=kappa, kernel=ratio, yardstick=yard))
            if not (err <= kappa * unit).all():
                failures.append(f'{name} row {b} contrast {m}: gamma {ratio:.2f} units > kappa {kappa} (fp32 numpy {yard:.2f})')
    assert not failures, '\n'.join(failures)
    # every flag at once = the three steps one after the other, to the bit; run against run; the generic kernel
    va = run(0xff)
    assert torch.equal(va.view(torch.int32), run(T.NOISE, run(T.GAMMA | T.INVERT, run(T.CONTRAST))).view(torch.int32))
    assert torch.equal(va.view(torch.int32), run(0xff).view(torch.int32))
    if M == 4:
        assert torch.equal(va.view(torch.int32), run(0xff, form=1).view(torch.int32))
    van = to_host(va)
    np.testing.assert_array_equal(van == -10, ref['x'] == -10, err_msg=f'{name}: the -10 markers')
    assert np.isfinite(van).all() and np.array_equal(van[3].view(np.uint32), yn[3].view(np.uint32)) and not np.array_equal(van[0], yn[0])
    if M > 1:
        assert np.array_equal(van[4, 1].view(np.uint32), yn[4, 1].view(np.uint32)) and (van[4, 1] == 0).all()      # the absent contrast stays zero
    assert (van[2] == yn[2]).all()                                  # blur only: nothing for the tone
    # the three calls in one
    x = to_dev(ref['x'])
    hip.launch_counts(reset=True)
    z = p.patch_intensify(x, tab, col, M)
    _counts(hip, patchblur=1, patchstats=1, patchtone=1, all=(2 if M == 4 else 3) + 2 + 1)
    assert torch.equal(z.view(torch.int32), va.view(torch.int32)) and torch.equal(x, to_dev(ref['x']))


def test_every_refusal_raises_before_any_launch(mrdis):
    hip, p = mrdis.hip, mrdis.patch3d
    M, patch = 4, (4, 4, 8)
    good = lambda: torch.zeros((2,) + patch + (M,), device=DEV).permute(0, 4, 1, 2, 3)
    tab = torch.zeros((2, 2 * M + 7 + p.TONE_EXTRA(M)), dtype=torch.int64, device=DEV)
    st = torch.zeros((2, M, 4), dtype=torch.int32, device=DEV)
    col = 2 * M + 7
    bad = [lambda: p.patch_blur(good().double(), tab, col, M), lambda: p.patch_blur(good().contiguous(), tab, col, M), lambda: p.patch_blur(good(), tab, col + 1, M),
           lambda: p.patch_blur(good(), tab, -1, M), lambda: p.patch_blur(good(), tab[:1], col, M), lambda: p.patch_blur(good(), tab.cpu(), col, M),
           lambda: p.patch_blur(good(), tab.int(), col, M), lambda: p.patch_blur(good(), tab, col, 3), lambda: p.patch_blur(good()[:, :, :, :, ::2], tab, col, M),
           lambda: p.patch_stats(good().half(), M), lambda: p.patch_stats(good(), 5), lambda: p.patch_stats(good().cpu().contiguous(), M),
           lambda: p.patch_tone(good(), st.float(), tab, col, M), lambda: p.patch_tone(good(), st[:, :3], tab, col, M), lambda: p.patch_tone(good(), st.cpu(), tab, col, M),
           lambda: p.patch_tone(good(), st, tab[:, :-1], col, M), lambda: p.patch_tone(good(), st, tab, col, 0), lambda: p.patch_intensify(good(), tab, 2.0, M),
           lambda: p.patch_intensify(good(), tab[:, ::2], 0, M)]
    hip.launch_counts(reset=True)
    for k, call in enumerate(bad):
        with pytest.raises(hip.MrdisError):
            call()
    assert hip.launch_counts()['all'] == 0 and not any(hip.launch_counts().values())
    # the library's own refusals of what the binding lets through: x == y, a workspace too small
    lib = hip.load()
    x = good()
    ws = torch.empty(lib.mrdis_patch_blur_workspace(2, M, *patch), dtype=torch.uint8, device=DEV)
    args = lambda y, n: (x.data_ptr(), y.data_ptr(), tab.data_ptr(), tab.shape[1], col, 2, M, *patch, ws.data_ptr(), n, None)
    assert lib.mrdis_patch_blur(*args(x, ws.numel())) < 0 and lib.mrdis_patch_blur(*args(good(), ws.numel() - 1)) < 0
    assert hip.launch_counts()['all'] == 0 and hip.launch_counts()['patchblur'] == 0


def test_three_calls_replay_through_a_graph_with_the_next_table(mrdis):
    p = mrdis.patch3d
    name = 'm4 slab'
    M, patch = CASES[name]
    ref = _case(name)
    x = to_dev(ref['x'])
    tabs = []
    for k in range(3):                                              # the case's blocks, the rows rotated: every row meets other flags and another seed
        t, col = _table(M, np.roll(ref['blocks'], k, axis=0), np.random.RandomState(k))
        tabs.append(t)
    eager = [p.patch_intensify(x, t, col, M) for t in tabs]
    assert not torch.equal(eager[0], eager[1])
    static = tabs[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        p.patch_intensify(x, static, col, M)                        # warm-up outside the capture (the workspace grows here)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = p.patch_intensify(x, static, col, M)
    for t, want in zip(tabs[1:] + tabs[:1], eager[1:] + eager[:1]):
        static.copy_(t)
        g.replay()
        assert torch.equal(out.view(torch.int32), want.view(torch.int32))


# ---------------------------------------------------------------- the loader
CONTRASTS = ['T1', 'T1c', 'T2', 'T2_FLAIR']
KEYS = dict(patch_blur=0.7, patch_blur_sigma=(0.4, 1.0), patch_contrast=0.6, patch_contrast_range=(0.6, 1.8), patch_gamma=0.6, patch_gamma_range=(0.6, 1.9),
            patch_gamma_invert=0.5, patch_noise=0.6, patch_noise_std=(0.05, 0.3))


@pytest.fixture(scope='module')
def loader_world():
    data = data3d_volumes(n_subj=5, H=12, W=16, D=24, contrasts=CONTRASTS, seed=13)
    for k in [k for k in data if k.endswith('/seg')]:
        seg = np.zeros_like(data[k])
        rs = np.random.RandomState(len(k) + int(k[-7:-4]))
        seg.reshape(-1)[rs.choice(seg.size, 200, replace=False)] = rs.choice([1, 2, 4], 200)
        data[k] = seg
    return data, data3d_subjects(data)


def _loader(mrdis, world, **kw):
    data, subj = world
    store = mrdis.VolumeStore3D.from_arrays(data, DEV)
    ds = mrdis.VolumeDataset3D('BraTS', store, subj, CONTRASTS, aug=kw.pop('aug', True), dropoff=True)
    return mrdis.VolumeLoader3D(ds, 2, shuffle=False, region_channels=3, **kw)


@pytest.mark.parametrize('step', ['blur', 'contrast', 'gamma', 'noise'])
def test_seeded_loader_gives_the_oracles_batches(mrdis, loader_world, step):
    """one share on at a time, so that every step meets the oracle's float64 composition of gather plus that step under its own bound; the
    gather is exact, and the statistics the tone steps use are those of the unblurred item, which the oracle computes itself"""
    hip = mrdis.hip
    data, subj = loader_world
    patch = (8, 8, 16)
    keys = dict(KEYS, **{k: 1.0 if k == 'patch_' + step else 0.0 for k in ('patch_blur', 'patch_contrast', 'patch_gamma', 'patch_noise')})
    kw = dict(patch_fg=0.5, patch_flips='hwd', **keys)
    la = _loader(mrdis, loader_world, patch_size=patch, **kw)
    assert la.dataset.intensifies()
    flagged = 0
    for epoch in range(2):
        np.random.seed(51 + epoch)
        list(la)                                                    # (prefix tables and minima are made outside the counted region)
        np.random.seed(51 + epoch)
        hip.launch_counts(reset=True)
        got = list(la)
        _counts(hip, patchorigin=3, patchgather=6, patchblur=3, patchstats=3, patchtone=3, all=3 + 6 + 3 * 2 + 3 * 2 + 3)
        twin = np.random.RandomState(51 + epoch)
        want = T.loader_batches(data, subj, CONTRASTS, 2, patch, twin, dropoff=True, K=3, **kw)
        assert np.random.get_state()[2] == twin.get_state()[2] and (np.random.get_state()[1] == twin.get_state()[1]).all()     # the same draws, no more
        assert len(got) == len(want) == 3
        for b, w in zip(got, want):
            assert b['inputs'].shape == (len(w['gathered']), 4) + patch and b['inputs'].permute(0, 2, 3, 4, 1).is_contiguous()
            np.testing.assert_array_equal(to_host(b['origins']), w['origins'])
            np.testing.assert_array_equal(to_host(b['targets']), w['targets'])
            np.testing.assert_array_equal(to_host(b['mask']), w['mask'])
            x = to_host(b['inputs'])
            np.testing.assert_array_equal(x == -10, w['gathered'] == -10)
            for i, tn in enumerate(w['tone']):
                seed, flags, sigma, f, gm, sd = tn
                gx = w['gathered'][i]
                st = T.stats(gx)
                for m in range(4):
                    if not flags[m]:
                        assert np.array_equal(x[i, m].view(np.uint32), gx[m].view(np.uint32)), (step, i, m)
                        continue
                    flagged += 1
                    assert w['mask'][i, m] == 1                     # an absent or dropped contrast carries no flag
                    if step == 'blur':
                        y64 = T.blur(gx, flags, np.stack([T.taps(s) for s in sigma]), np.float64)
                        assert (np.abs(x[i, m].astype(np.float64) - y64[m]) <= T.blur_bound(gx)[m]).all()
                    elif step == 'noise':
                        assert np.array_equal(x[i, m].view(np.uint32), T.tone(gx, st, flags, f, gm, sd, seed, np.float32)[m].view(np.uint32))
                    else:
                        v64 = T.tone(gx, st, flags, f, gm, sd, seed, np.float64)[m]
                        if step == 'contrast':            # (the kernel's mean may sit one fp32 ulp from the oracle's: |1 - f| of it reaches v)
                            bound = T.contrast_bound(st[0][m], st[1][m], f[m]) + abs(1 - float(f[m])) * float(np.spacing(np.abs(st[2][m])))
                        else:
                            yard = np.abs(T.tone(gx, st, flags, f, gm, sd, seed, np.float32)[m].astype(np.float64) - v64).max() / T.gamma_unit(st[0][m], st[1][m])
                            bound = max(4, math.ceil(4 * yard)) * T.gamma_unit(st[0][m], st[1][m])
                        assert (np.abs(x[i, m].astype(np.float64) - v64) <= bound).all(), (step, i, m)
    assert flagged >= 8


def test_loader_with_every_share_and_the_warp_equals_the_direct_calls(mrdis, loader_world):
    """the composition on a warping loader: its table is the oracle's packing of the oracle's draws at the column after the warp words, and
    its inputs are patch_intensify of patch_warp under that table, to the bit"""
    hip, p = mrdis.hip, mrdis.patch3d
    data, subj = loader_world
    patch = (8, 8, 16)
    kw = dict(patch_fg=0.5, patch_flips='hwd', patch_warp=0.5, **dict(KEYS, patch_blur=1.0, patch_noise=1.0))
    la = _loader(mrdis, loader_world, patch_size=patch, **kw)
    st = la.dataset.store
    np.random.seed(61)
    list(la)
    np.random.seed(61)
    plans = list(la.batch_plan())
    np.random.seed(61)
    hip.launch_counts(reset=True)
    got = list(la)
    _counts(hip, patchorigin=3, patchwarp=6, patchblur=3, patchstats=3, patchtone=3, all=3 + 6 + 3 * 2 + 3 * 2 + 3)
    twin = np.random.RandomState(61)
    col = 2 * 4 + 12
    assert la.dataset.tone_col() == col
    seen = 0
    for b, (_, _, metas) in zip(got, plans):
        tab = la.patch_table(metas)[0]
        assert tab.shape == (len(metas), col + p.TONE_EXTRA(4))
        for r, m in enumerate(metas):
            present = [data.get(m[0] + '/' + c) is not None for c in CONTRASTS]
            tn = T.draw_item(twin, present, True, True, 0.5, 'hwd', 0.5, **{k: v for k, v in kw.items() if k in T.DEFAULTS})[7]
            assert np.array_equal(tab[r, col:], T.pack(*tn))
            seen += sum(1 for f in tn[1] if f)
        d = torch.from_numpy(tab).to(DEV)
        o = p.patch_origins(d, 4, st.shape, patch, (1, 2, 4))
        x, mask = p.patch_warp(d, o, 4, st.shape, patch)
        assert torch.equal(b['inputs'].view(torch.int32), p.patch_intensify(x, d, col, 4).view(torch.int32)) and torch.equal(b['mask'], mask)
        assert torch.equal(b['targets'], p.patch_warp(d, o, 4, st.shape, patch, targets=True, K=3, relabel=True))
        assert torch.equal(b['inputs'] == -10, x == -10) and not torch.equal(b['inputs'], x)
    assert seen >= 10


def test_shares_at_zero_leave_batches_streams_and_counts_as_they_were(mrdis, loader_world):
    hip = mrdis.hip
    data, subj = loader_world
    patch = (8, 8, 16)
    kw = dict(patch_fg=0.5, patch_flips='hwd')
    off = _loader(mrdis, loader_world, patch_size=patch, patch_blur=0.0, patch_contrast=0.0, patch_gamma=0.0, patch_noise=0.0, patch_blur_sigma=(1, 1), patch_gamma_invert=1.0, **kw)
    assert not off.dataset.intensifies()
    np.random.seed(71)
    list(off)
    np.random.seed(71)
    hip.launch_counts(reset=True)
    got = list(off)
    _counts(hip, patchorigin=3, patchgather=6, all=9)               # no new counter above 0
    twin = np.random.RandomState(71)
    want = chk.loader_batches(data, subj, CONTRASTS, 2, patch, twin, aug=True, dropoff=True, K=3, **kw)
    assert np.random.get_state()[2] == twin.get_state()[2] and (np.random.get_state()[1] == twin.get_state()[1]).all()
    for b, w in zip(got, want):
        np.testing.assert_array_equal(to_host(b['inputs']), w['inputs'])
        np.testing.assert_array_equal(to_host(b['targets']), w['targets'])
        np.testing.assert_array_equal(to_host(b['origins']), w['origins'])
    # the evaluation loaders never intensify
    ev = _loader(mrdis, loader_world, aug=False, patch_size=patch, patch_centre=True, **KEYS)
    hip.launch_counts(reset=True)
    assert len(list(ev)) == 3
    _counts(hip, patchorigin=3, patchgather=6, all=9)


# ---------------------------------------------------------------- Run3D
@pytest.fixture(scope='module')
def run_world(tmp_path_factory):
    data = data3d_volumes(n_subj=11, H=32, W=48, D=40, contrasts=CONTRASTS, seed=17)
    subj = data3d_subjects(data)
    root = tmp_path_factory.mktemp('tone3d')
    for name, part in (('train', subj[:5]), ('val', subj[5:8]), ('test', subj[8:11])):
        (root / f'fold_BraTS_3d_0_{name}_noval.txt').write_text('\n'.join(part) + '\n')
    return data, str(root), subj


def _run3d(mrdis, world, ckpt, **over):
    cfg = dict(dataset_name='BraTS', data_path=world[1], contrast_list=CONTRASTS, batch_size=2, model_name='NVNet3D', init_channels=8, epochs=2, lr=1e-4,
               ckpt_path=str(ckpt), device='cuda:0', seed=10, patch_size=[16, 16, 16], patch_fg=0.5, patch_flips='hwd')
    cfg.update(over)
    return mrdis.Run3D(cfg, store=mrdis.VolumeStore3D.from_arrays(world[0], DEV), log=lambda *a: None)


def test_run3d_trains_and_resumes_with_the_keys_on(mrdis, run_world, tmp_path):
    hip = mrdis.hip
    on = {k: (list(v) if isinstance(v, tuple) else v) for k, v in KEYS.items()}
    straight = _run3d(mrdis, run_world, tmp_path / 'straight', **on)
    tr, va = straight.loaders['train'].dataset, straight.loaders['val'].dataset
    assert tr.intensifies() and tr.intensity['patch_blur'] == 0.7 and not va.intensifies() and not straight.loaders['test'].dataset.intensifies()
    hip.launch_counts(reset=True)
    straight.train()
    c = hip.launch_counts()
    steps, vals = len(straight.loaders['train']), len(straight.loaders['val'])
    assert steps == 2 and vals == 1
    assert c['patchblur'] == c['patchstats'] == c['patchtone'] == 2 * steps and c['patchgather'] == 4 * (steps + vals) and c['patchwarp'] == 0, c
    assert 0 < straight.last_stat['dice'] < 1 and np.isfinite(straight.last_stat['loss'])
    first = _run3d(mrdis, run_world, tmp_path / 'resumed', **on)
    first._train(1)                                                            # an interrupted run
    del first
    second = _run3d(mrdis, run_world, tmp_path / 'resumed', continue_train=True, **on)
    assert second.start_epoch == 0
    second.train()
    a, b = straight.model.state_dict(), second.model.state_dict()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert straight.last_stat == second.last_stat
    # the default keys: no new counter above 0, and another training
    hip.launch_counts(reset=True)
    default = _run3d(mrdis, run_world, tmp_path / 'default')
    default.train()
    c = hip.launch_counts()
    assert c['patchblur'] == c['patchstats'] == c['patchtone'] == 0 and c['patchgather'] > 0, c
    assert any(not torch.equal(a[k], v) for k, v in default.model.state_dict().items())       # (the feature does reach the training batches)
