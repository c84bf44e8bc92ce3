"""Region scoring on the GPU: the kernels of csrc/mrdis_surfdist.hip (hip.region_surfaces, hip.edt_sq / mrdis.edt3d_sq, hip.surface_hist),
mrdis.region_scores and `Run3D` with predict_regions / phase=score.

Everything is integer arithmetic, so every comparison is for equality.  The oracle of the distance transform is an independent brute force in
numpy int64: for every voxel that is not a feature, the minimum over ALL features of the squared coordinate difference (chunked; a case stays
under about 5e7 voxel-feature pairs).  Which shape takes which path (see the header of mrdis_surfdist.hip):
  (1,5,7,9) (1,1,1,1) (1,1,1,64)   one step of the D scan, one d tile, lines shorter than the four-output groups of the min-plus passes
  (2,33,17,70)                     a D line that crosses a 64-voxel step (carry both ways), two d tiles (the second 6 wide), two batch items
  (1,2,3,257) (1,257,2,3) (1,3,257,2)   one axis longer than a 256-thread block: five scan steps / a min-plus line of 257 (H or W)
  (1,256,2,3) (1,3,256,2)          a min-plus line of 256: the LDS tile is exactly 64 KB, and the kernel's static LDS comes on top of it
region_surfaces: H W D = 5 x 6 x 9 = 270 and 3 x 5 x 70 = 1050 (both % 4 = 2): with B = 3 the samples start at voxel phases 0, 2, 0, so the
vector groups inside a sample and the element groups at its ends both run; D = 9 and 70 are no multiple of 16.
The scores other than hd95 are ratios of exact integers formed in float64 by two different expressions: within 1e-15."""
import math
import os

import numpy as np
import pytest
import torch

from fixtures_data3d import data3d_volumes, data3d_subjects

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
FAR = 1 << 30
BRATS_MASKS = (0b10110, 0b10010, 0b10000)


@pytest.fixture(scope='module')
def mrdis():
    import mrdis as m
    return m


# ----------------------------------------------------------------------------------------------- oracles (numpy, CPU)
def brute_edt_sq(mask):
    """(H, W, D) bool -> int64 squared distance to the nearest True voxel, FAR without one: the minimum over all features, no separability"""
    mask = np.asarray(mask, dtype=bool)
    out = np.zeros(mask.shape, dtype=np.int64)
    feat = np.argwhere(mask).astype(np.int64)
    if len(feat) == 0:
        out[...] = FAR
        return out
    rest = np.argwhere(~mask).astype(np.int64)
    step = max(1, 4_000_000 // len(feat))
    for a in range(0, len(rest), step):
        r = rest[a:a + step]
        d2 = ((r[:, None, :] - feat[None, :, :]) ** 2).sum(-1).min(1)
        out[r[:, 0], r[:, 1], r[:, 2]] = d2
    return out


def np_nibbles(vol, masks):
    """(...) label values (float or int) -> (R, ...) bool membership; values above 7, negative or non-integral belong to no region"""
    v = np.asarray(vol, dtype=np.float64)
    ok = (v >= 0) & (v <= 7) & (v == np.floor(v))
    l = np.where(ok, v, 0).astype(np.int64)
    return np.stack([ok & (((m >> l) & 1) == 1) for m in masks])


def np_surface(inside):
    """(..., H, W, D) bool -> surface voxels: inside with a face neighbour outside, the border counting as outside"""
    p = np.pad(inside, [(0, 0)] * (inside.ndim - 3) + [(1, 1)] * 3)
    core = p[..., 1:-1, 1:-1, 1:-1]
    allnb = (p[..., :-2, 1:-1, 1:-1] & p[..., 2:, 1:-1, 1:-1] & p[..., 1:-1, :-2, 1:-1] & p[..., 1:-1, 2:, 1:-1]
             & p[..., 1:-1, 1:-1, :-2] & p[..., 1:-1, 1:-1, 2:])
    return core & ~allnb


def np_flags_counts(labels, targets, masks, has_target=None):
    """labels (B, H, W, D) uint8, targets (B, H, W, D) float -> flags (B, H, W, D) uint8, counts (B, R, 5) int64"""
    B = labels.shape[0]
    P = np_nibbles(labels, masks)                                    # (R, B, H, W, D)
    T = np_nibbles(targets, masks)
    if has_target is not None:
        T = T & np.asarray(has_target, dtype=bool)[None, :, None, None, None]
    sP, sT = np_surface(P), np_surface(T)
    flags = np.zeros(labels.shape, dtype=np.uint8)
    counts = np.zeros((B, len(masks), 5), dtype=np.int64)
    for r in range(len(masks)):
        flags |= (sP[r].astype(np.uint8) << r) | (sT[r].astype(np.uint8) << (4 + r))
        for k, a in enumerate((P[r] & T[r], P[r], T[r], sP[r], sT[r])):
            counts[:, r, k] = a.reshape(B, -1).sum(1)
    return flags, counts


def nearest_d2(at, src, shape, rho):
    """squared distance from every voxel of `at` (n, 3) to the nearest of `src` (m, 3).  rho None: brute force over all pairs.  Otherwise the
    minimum over the features inside the cube of half-width rho around the voxel first -- exact whenever it is <= rho^2, since every voxel
    outside the cube is further than rho away -- and the brute force over all features for the voxels that leaves open."""
    if rho is None:
        return ((at[:, None, :] - src[None, :, :]) ** 2).sum(-1).min(1)
    vol = np.zeros(tuple(n + 2 * rho for n in shape), dtype=bool)
    vol[src[:, 0] + rho, src[:, 1] + rho, src[:, 2] + rho] = True
    best = np.full(len(at), np.iinfo(np.int64).max, dtype=np.int64)
    for dh in range(-rho, rho + 1):
        for dw in range(-rho, rho + 1):
            for dd in range(-rho, rho + 1):
                hit = vol[at[:, 0] + rho + dh, at[:, 1] + rho + dw, at[:, 2] + rho + dd]
                best = np.where(hit, np.minimum(best, dh * dh + dw * dw + dd * dd), best)
    todo = np.nonzero(best > rho * rho)[0]
    for a in range(0, len(todo), 64):
        i = todo[a:a + 64]
        best[i] = ((at[i][:, None, :] - src[None, :, :]) ** 2).sum(-1).min(1)
    return best


def np_hist(flags, R, bins, rho=None):
    """hist (B, R, 2, bins) int64 by brute force over the surface voxels (`rho`: see nearest_d2; for dense surfaces in a large volume)"""
    B = flags.shape[0]
    hist = np.zeros((B, R, 2, bins), dtype=np.int64)
    for b in range(B):
        for r in range(R):
            sp = np.argwhere((flags[b] >> r) & 1).astype(np.int64)
            st = np.argwhere((flags[b] >> (4 + r)) & 1).astype(np.int64)
            for direction, (at, src) in enumerate(((st, sp), (sp, st))):
                if len(at) and len(src):
                    hist[b, r, direction] = np.bincount(nearest_d2(at, src, flags.shape[1:], rho), minlength=bins)
    return hist


def np_scores(counts, hist, shape, spacing, has_target=None):
    """the scoring rules of surfdist.region_scores written out per sample and region in plain Python"""
    B, R = counts.shape[:2]
    H, W, D = shape
    N = H * W * D
    out = {k: np.zeros((B, R)) for k in ('dice', 'sensitivity', 'specificity', 'hd95')}
    for b in range(B):
        for r in range(R):
            I, P, T, nP, nT = (int(x) for x in counts[b, r])
            if has_target is not None and not has_target[b]:
                for k in out:
                    out[k][b, r] = float('nan')
                continue
            out['sensitivity'][b, r] = I / T if T else 1.0
            out['specificity'][b, r] = (N - P - T + I) / (N - T) if N != T else 1.0
            if P == 0 and T == 0:
                out['dice'][b, r], out['hd95'][b, r] = 1.0, 0.0
            elif P == 0 or T == 0:
                out['dice'][b, r], out['hd95'][b, r] = 0.0, spacing * math.sqrt(H * H + W * W + D * D)
            else:
                out['dice'][b, r] = 2 * I / (P + T)
                ks = []
                for direction, n in ((0, nT), (1, nP)):
                    cum = np.cumsum(hist[b, r, direction])
                    assert cum[-1] == n
                    ks.append(int(np.nonzero(20 * cum >= 19 * n)[0][0]))
                out['hd95'][b, r] = spacing * math.sqrt(max(ks))
    return out


# ----------------------------------------------------------------------------------------------- edt3d_sq
SMALL = [(1, 5, 7, 9), (1, 1, 1, 1), (1, 1, 1, 64)]
SHAPES = SMALL + [(2, 33, 17, 70), (1, 2, 3, 257), (1, 257, 2, 3), (1, 3, 257, 2), (1, 256, 2, 3), (1, 3, 256, 2)]
PATTERNS = ('half', 'sparse', 'corner', 'far_end', 'ones', 'zeros', 'item0_empty')


def make_mask(shape, pattern, seed=5):
    rng = np.random.RandomState(seed)
    m = np.zeros(shape, dtype=bool)
    if pattern == 'half':
        m = rng.rand(*shape) < 0.5
    elif pattern == 'sparse':
        m = rng.rand(*shape) < 0.02
    elif pattern == 'corner':
        m[:, 0, 0, 0] = True
    elif pattern == 'far_end':                                       # the far end of the longest axis, the other coordinates at their last voxel too
        m[:, -1, -1, -1] = True
    elif pattern == 'ones':
        m[...] = True
    elif pattern == 'item0_empty':                                   # a leak across the batch would give item 0 finite distances
        m[-1] = rng.rand(*shape[1:]) < 0.02
        m[-1, shape[1] // 2, shape[2] // 2, shape[3] // 2] = True
        m[0] = False
    return m


EDT_CASES = [(s, p) for s in SHAPES for p in PATTERNS if not (p == 'half' and s not in SMALL)]


@pytest.mark.parametrize('shape,pattern', EDT_CASES, ids=['x'.join(map(str, s)) + '-' + p for s, p in EDT_CASES])
def test_edt3d_sq_equals_the_brute_force(mrdis, shape, pattern):
    m = make_mask(shape, pattern)
    if pattern == 'item0_empty' and shape[0] == 1:
        m = np.concatenate([np.zeros_like(m), m])                    # every shape gets a two-item batch: item 0 empty, item 1 not
        m[1].flat[0] = True
    want = np.stack([brute_edt_sq(x) for x in m])
    got = mrdis.edt3d_sq(torch.from_numpy(m).to(DEV))
    assert got.dtype == torch.int32 and tuple(got.shape) == m.shape
    got = got.cpu().numpy().astype(np.int64)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    if pattern == 'zeros':
        assert (got == mrdis.EDT_FAR).all()
    if pattern == 'item0_empty':
        assert (got[0] == mrdis.EDT_FAR).all() and got[1].max() < mrdis.EDT_FAR
    # a uint8 mask (any non-zero byte is a feature) and a single (H, W, D) volume give the same integers
    u8 = torch.from_numpy(m.astype(np.uint8) * 37).to(DEV)
    assert torch.equal(mrdis.edt3d_sq(u8).cpu(), torch.from_numpy(got.astype(np.int32)))
    assert torch.equal(mrdis.edt3d_sq(u8[-1]).cpu(), torch.from_numpy(got[-1].astype(np.int32)))


def test_edt_of_flag_bits_transforms_every_source_in_one_call(mrdis):
    rng = np.random.RandomState(8)
    shape = (2, 9, 11, 70)
    flags = (rng.randint(0, 256, shape) * (rng.rand(*shape) < 0.05)).astype(np.uint8)
    bits = (0, 3, 4, 7)
    before = mrdis.hip.launch_counts()
    got = mrdis.hip.edt_sq(torch.from_numpy(flags).to(DEV), [1 << k for k in bits]).cpu().numpy()
    after = mrdis.hip.launch_counts()
    assert after['edt'] - before['edt'] == 3 and after['surfhist'] == before['surfhist']
    assert got.shape == (4,) + shape
    for s, k in enumerate(bits):
        want = np.stack([brute_edt_sq((x >> k) & 1) for x in flags])
        assert np.array_equal(got[s], want), k


def test_unsupported_extents_are_refused(mrdis):
    for shape in ((1, 1025, 2, 2), (1, 2, 1025, 2), (1, 2, 2, 1025), (1, 0, 2, 2), (1, 2, 0, 2), (1, 2, 2, 0), (0, 2, 2, 2)):
        with pytest.raises(mrdis.MrdisError, match='unsupported geometry'):
            mrdis.edt3d_sq(torch.zeros(shape, dtype=torch.uint8, device=DEV))
    with pytest.raises(mrdis.MrdisError, match='unsupported geometry'):
        mrdis.region_scores(torch.zeros((1, 1025, 2, 2), dtype=torch.uint8, device=DEV), None)
    with pytest.raises(mrdis.MrdisError):
        mrdis.edt3d_sq(torch.zeros((1, 2, 2, 2), dtype=torch.float32, device=DEV))
    with pytest.raises(mrdis.MrdisError):
        mrdis.hip.edt_sq(torch.zeros((1, 2, 2, 4), dtype=torch.uint8, device=DEV)[..., ::2])          # not contiguous
    for bad in ([256], [-1], [], [1] * 9):
        with pytest.raises(mrdis.MrdisError):
            mrdis.hip.edt_sq(torch.zeros((1, 2, 2, 2), dtype=torch.uint8, device=DEV), bad)              # source masks are bytes, 1 .. 8 of them
    lib = mrdis.hip.load()
    buf = torch.zeros(64, dtype=torch.int32, device=DEV)
    for H, W, D in ((1025, 1, 1), (1, 1025, 1), (1, 1, 1025), (0, 1, 1)):
        assert lib.mrdis_edt_sq(buf.data_ptr(), b'\xff', 1, buf.data_ptr(), buf.data_ptr(), 256, 1, H, W, D, None) == -1      # MRDIS_EINVAL, nothing launched


# ----------------------------------------------------------------------------------------------- region_surfaces
def random_labels(shape, seed, blobs=False):
    """(labels uint8, targets fp32): values from {0, 1, 2, 4} plus some 3 and 9; the targets also hold a few non-integral and negative values"""
    rng = np.random.RandomState(seed)
    if blobs:                                                        # nested ellipsoids, prediction and ground truth a little apart
        B, H, W, D = shape
        g = np.stack(np.meshgrid(np.arange(H), np.arange(W), np.arange(D), indexing='ij')).astype(np.float64)
        vols = []
        for shift in (0.0, 1.3):
            v = np.zeros(shape, dtype=np.uint8)
            for b in range(B):
                c = np.array([H, W, D]) * (0.5 + 0.08 * rng.randn(3)) + shift
                rad = np.array([H, W, D]) * (0.33 + 0.05 * rng.rand(3))
                q = (((g - c[:, None, None, None]) / rad[:, None, None, None]) ** 2).sum(0)
                v[b][q < 1.0] = 2
                v[b][q < 0.45] = 1
                v[b][q < 0.2] = 4
            vols.append(v)
        labels, targets = vols[0], vols[1].astype(np.float32)
    else:
        vals = np.array([0, 1, 2, 4, 3, 9], dtype=np.uint8)
        prob = [0.3, 0.2, 0.2, 0.2, 0.05, 0.05]
        labels = rng.choice(vals, size=shape, p=prob)
        targets = rng.choice(vals, size=shape, p=prob).astype(np.float32)
        odd = rng.rand(*shape) < 0.03
        targets[odd] = rng.choice(np.array([1.5, -1.0, 0.25, 200.0, 7.0], dtype=np.float32), size=int(odd.sum()))
    return labels, targets


def run_region_surfaces(mrdis, labels, targets, masks, has_target=None):
    lab = torch.from_numpy(labels).to(DEV)
    tgt = torch.from_numpy(targets).to(DEV)
    step = targets[0].size * 4
    ptrs = [tgt.data_ptr() + b * step if (has_target is None or has_target[b]) else 0 for b in range(labels.shape[0])]
    flags, counts = mrdis.hip.region_surfaces(lab, torch.tensor(ptrs, dtype=torch.int64).to(DEV), masks)
    torch.cuda.synchronize()
    return flags, counts, tgt


@pytest.mark.parametrize('shape,blobs', [((3, 5, 6, 9), False), ((3, 3, 5, 70), False), ((2, 12, 10, 9), True), ((1, 4, 4, 16), False)],
                         ids=['d9', 'd70', 'blobs', 'vector-only'])
def test_region_surfaces_flags_and_counts_equal_numpy(mrdis, shape, blobs):
    labels, targets = random_labels(shape, seed=21, blobs=blobs)
    labels[0, :2, :, :] = 4                                          # a region that touches the volume border: its border voxels are surface
    targets[0, :, :, -3:] = 1.0
    has_target = [True] * shape[0]
    if shape[0] > 1:
        has_target[1] = False                                        # a zero target pointer: ground-truth bits and T counts stay 0
    want_flags, want_counts = np_flags_counts(labels, targets, BRATS_MASKS, has_target)
    flags, counts, _ = run_region_surfaces(mrdis, labels, targets, BRATS_MASKS, has_target)
    assert flags.dtype == torch.uint8 and counts.dtype == torch.int32 and tuple(counts.shape) == (shape[0], 3, 5)
    assert np.array_equal(flags.cpu().numpy(), want_flags)
    assert np.array_equal(counts.cpu().numpy().astype(np.int64), want_counts)
    assert want_counts[0, :, 3].min() > 0 and (want_flags[0, 0] & 1).all()           # the border slab of label 4: every voxel of the face is WT surface
    if shape[0] > 1:
        assert (want_flags[1] >> 4).max() == 0 and want_counts[1, :, 2].max() == 0 and want_counts[1, :, 4].max() == 0
    # no pointer table at all: no ground truth for any sample
    f2, c2 = mrdis.hip.region_surfaces(torch.from_numpy(labels).to(DEV), None, BRATS_MASKS)
    assert np.array_equal(f2.cpu().numpy(), want_flags & 15) and int(c2[:, :, [0, 2, 4]].abs().max()) == 0
    assert np.array_equal(c2[:, :, [1, 3]].cpu().numpy(), want_counts[:, :, [1, 3]])


# ----------------------------------------------------------------------------------------------- surface_hist / region_scores
@pytest.fixture(scope='module')
def scored(mrdis):
    """one region_scores call on blobs (B = 3, sample 2 without ground truth) with its oracle, shared by the tests below"""
    shape = (3, 12, 10, 70)
    labels, targets = random_labels(shape, seed=33, blobs=True)
    labels[1][labels[1] == 4] = 1                                    # sample 1 predicts no enhancing tumour: ET is empty on one side
    has_target = [True, True, False]
    lab = torch.from_numpy(labels).to(DEV)
    tgt = torch.from_numpy(targets).to(DEV)
    step = targets[0].size * 4
    ptrs = torch.tensor([tgt.data_ptr() + b * step if has_target[b] else 0 for b in range(3)], dtype=torch.int64).to(DEV)
    before = mrdis.hip.launch_counts()
    res = mrdis.region_scores(lab, ptrs, spacing=1.25)
    after = mrdis.hip.launch_counts()
    launches = {k: after[k] - before[k] for k in mrdis.hip.SURFDIST_FAMILIES}
    flags, counts = np_flags_counts(labels, targets, BRATS_MASKS, has_target)
    bins = mrdis.hip.edt_bins(*shape[1:])
    hist = np_hist(flags, 3, bins)
    return dict(labels=labels, targets=targets, lab=lab, tgt=tgt, ptrs=ptrs, res=res, launches=launches, flags=flags, counts=counts, hist=hist,
                bins=bins, shape=shape, has_target=has_target)


def test_surface_hist_equals_numpy(mrdis, scored):
    s = scored
    flags, counts = mrdis.hip.region_surfaces(s['lab'], s['ptrs'], BRATS_MASKS)
    assert np.array_equal(flags.cpu().numpy(), s['flags'])
    hist = mrdis.hip.surface_hist(flags, 3)
    assert hist.dtype == torch.int32 and tuple(hist.shape) == (3, 3, 2, s['bins'])
    got = hist.cpu().numpy().astype(np.int64)
    assert np.array_equal(got, s['hist'])
    assert s['hist'][0].sum() > 0
    assert got[1, 2].sum() == 0 and got[2].sum() == 0                # ET of sample 1 has an empty side, sample 2 no ground truth: nothing added
    # every measured voxel is counted once: row totals = the surface counts of the measured side, when both sides are non-empty
    for b in range(2):
        for r in range(3):
            if s['counts'][b, r, 3] and s['counts'][b, r, 4]:
                assert got[b, r, 0].sum() == s['counts'][b, r, 4] and got[b, r, 1].sum() == s['counts'][b, r, 3]


def test_surface_hist_beyond_the_lds_bins(mrdis):
    """two single voxels far apart: the one squared distance lies above the sub-histogram's 256 bins and goes straight to memory"""
    labels = np.zeros((1, 6, 7, 40), dtype=np.uint8)
    targets = np.zeros((1, 6, 7, 40), dtype=np.float32)
    labels[0, 1, 1, 2] = 4
    targets[0, 4, 5, 37] = 4.0
    flags, counts, _ = run_region_surfaces(mrdis, labels, targets, BRATS_MASKS)
    got = mrdis.hip.surface_hist(flags, 3).cpu().numpy()
    d2 = 9 + 16 + 35 * 35
    want = np.zeros_like(got)
    want[0, :, :, d2] = 1
    assert d2 > 256 and np.array_equal(got, want)


def test_surface_hist_of_distant_slabs_on_a_line_of_256(mrdis):
    """two slabs 186 voxels apart along H = 256 (a 64 KB tile plus the sub-histogram's static LDS): every squared distance lies beyond the
    sub-histogram, and many surface voxels add into the same bin of global memory"""
    shape = (1, 256, 5, 6)
    labels = np.zeros(shape, dtype=np.uint8)
    targets = np.zeros(shape, dtype=np.float32)
    labels[0, 10:15] = 4
    targets[0, 200:205] = 4.0
    flags, counts, _ = run_region_surfaces(mrdis, labels, targets, BRATS_MASKS)
    want_flags, want_counts = np_flags_counts(labels, targets, BRATS_MASKS)
    assert np.array_equal(flags.cpu().numpy(), want_flags) and np.array_equal(counts.cpu().numpy().astype(np.int64), want_counts)
    bins = mrdis.hip.edt_bins(*shape[1:])
    want = np_hist(want_flags, 3, bins)
    got = mrdis.hip.surface_hist(flags, 3).cpu().numpy().astype(np.int64)
    assert want[..., :256].sum() == 0 and want[0, 0, 0, 186 * 186] > 16 and want.sum() == 3 * 2 * want_counts[0, 0, 3]
    assert np.array_equal(got, want)
    res = mrdis.region_scores(torch.from_numpy(labels).to(DEV), torch.from_numpy(targets).to(DEV))
    assert res['hd95'].numpy().tobytes() == np_scores(want_counts, want, shape[1:], 1.0)['hd95'].tobytes()
    assert float(res['hd95'][0, 0]) >= 186.0


def test_region_scores_equal_the_oracle(mrdis, scored):
    s = scored
    res = s['res']
    assert res['names'] == ('wt', 'tc', 'et')
    assert res['counts'].dtype == torch.int64 and np.array_equal(res['counts'].numpy(), s['counts'])
    want = np_scores(s['counts'], s['hist'], s['shape'][1:], 1.25, s['has_target'])
    for k in ('dice', 'sensitivity', 'specificity', 'hd95'):
        assert res[k].dtype == torch.float64 and res[k].device.type == 'cpu' and tuple(res[k].shape) == (3, 3)
        assert bool(torch.isnan(res[k][2]).all())                    # no ground truth: NaN in all four
    got_hd, want_hd = res['hd95'][:2].numpy(), want['hd95'][:2]
    assert got_hd.tobytes() == want_hd.tobytes(), (got_hd, want_hd)  # bit-equal float64
    for k in ('dice', 'sensitivity', 'specificity'):
        assert np.abs(res[k][:2].numpy() - want[k][:2]).max() <= 1e-15, k
    diag = 1.25 * math.sqrt(12 ** 2 + 10 ** 2 + 70 ** 2)
    assert float(res['hd95'][1, 2]) == diag and float(res['dice'][1, 2]) == 0.0            # exactly one side empty
    assert 0 < float(res['hd95'][0, 0]) < diag and 0 < float(res['dice'][0, 0]) < 1
    # a tensor of targets (fp32 or uint8) instead of the pointer table: the same scores for the samples that have ground truth
    for tg in (s['tgt'], s['tgt'].to(torch.uint8)):
        r2 = mrdis.region_scores(s['lab'][:2].contiguous(), tg[:2].contiguous(), spacing=1.25)
        for k in ('dice', 'sensitivity', 'specificity', 'hd95'):
            assert torch.equal(r2[k], res[k][:2]), k
    r3 = mrdis.region_scores(s['lab'], None)
    assert all(bool(torch.isnan(r3[k]).all()) for k in ('dice', 'sensitivity', 'specificity', 'hd95'))


def box_volume(shift=(0, 0, 0), empty=False):
    v = np.zeros((1, 16, 18, 20), dtype=np.uint8)
    if not empty:
        v[0, 4 + shift[0]:10 + shift[0], 5 + shift[1]:11 + shift[1], 6 + shift[2]:12 + shift[2]] = 1
    return v


def test_analytic_boxes(mrdis):
    """a solid 6 x 6 x 6 box in a 16 x 18 x 20 volume"""
    regions = (('box', (1,)),)
    gt = torch.from_numpy(box_volume()).to(DEV)

    def score(pred, spacing=1.0):
        return mrdis.region_scores(torch.from_numpy(pred).to(DEV), gt, regions=regions, spacing=spacing)
    same = score(box_volume())
    assert float(same['dice']) == 1.0 and float(same['hd95']) == 0.0 and float(same['sensitivity']) == 1.0 and float(same['specificity']) == 1.0
    assert same['counts'].tolist() == [[[216, 216, 216, 216 - 64, 216 - 64]]]
    for axis in range(3):
        shift = tuple(3 if a == axis else 0 for a in range(3))
        r = score(box_volume(shift))
        assert float(r['hd95']) == 3.0, axis                          # a face moved by 3: more than 5 % of either surface is 3 away
        assert float(r['dice']) == 2 * 108 / 432 and float(r['sensitivity']) == 0.5
        assert float(score(box_volume(shift), spacing=2.0)['hd95']) == 6.0
    empty = score(box_volume(empty=True))
    assert float(empty['hd95']) == math.sqrt(16 ** 2 + 18 ** 2 + 20 ** 2) and float(empty['dice']) == 0.0 and float(empty['sensitivity']) == 0.0
    both = mrdis.region_scores(torch.from_numpy(box_volume(empty=True)).to(DEV), torch.from_numpy(box_volume(empty=True)).to(DEV), regions=regions)
    assert float(both['hd95']) == 0.0 and float(both['dice']) == 1.0 and float(both['sensitivity']) == 1.0 and float(both['specificity']) == 1.0


@pytest.mark.parametrize('regions', [(('core', (1, 4)),), (('a', (1,)), ('b', (2, 3)), ('c', (0,)), ('d', (1, 2, 3, 4, 7)))], ids=['R1', 'R4'])
def test_custom_regions(mrdis, regions):
    shape = (2, 7, 9, 21)
    labels, targets = random_labels(shape, seed=3)
    _, masks = mrdis.region_masks(regions)
    R = len(masks)
    res = mrdis.region_scores(torch.from_numpy(labels).to(DEV), torch.from_numpy(targets).to(DEV), regions=regions, spacing=0.5)
    flags, counts = np_flags_counts(labels, targets, masks)
    hist = np_hist(flags, R, mrdis.hip.edt_bins(*shape[1:]))
    want = np_scores(counts, hist, shape[1:], 0.5)
    assert res['names'] == tuple(n for n, _ in regions) and np.array_equal(res['counts'].numpy(), counts)
    assert res['hd95'].numpy().tobytes() == want['hd95'].tobytes()
    for k in ('dice', 'sensitivity', 'specificity'):
        assert np.abs(res[k].numpy() - want[k]).max() <= 1e-15, k
    got_hist = mrdis.hip.surface_hist(mrdis.hip.region_surfaces(torch.from_numpy(labels).to(DEV), None, masks)[0], R)
    assert int(got_hist.abs().max()) == 0                            # no ground truth: nothing to measure


def test_launch_counters_do_not_depend_on_the_batch_and_runs_repeat(mrdis, scored):
    s = scored
    assert s['launches'] == {'regsurf': 1, 'edt': 2, 'surfhist': 1}                   # B = 3
    runs = []
    for _ in range(2):
        before = mrdis.hip.launch_counts()
        res = mrdis.region_scores(s['lab'][:1].contiguous(), s['ptrs'][:1].contiguous(), spacing=1.25)
        after = mrdis.hip.launch_counts()
        assert {k: after[k] - before[k] for k in mrdis.hip.SURFDIST_FAMILIES} == s['launches']      # B = 1: the same counts
        runs.append(res)
    for k in ('dice', 'sensitivity', 'specificity', 'hd95', 'counts'):
        assert torch.equal(runs[0][k], runs[1][k]) and torch.equal(runs[0][k][0], s['res'][k][0]), k
    flags, _ = mrdis.hip.region_surfaces(s['lab'], s['ptrs'], BRATS_MASKS)
    a, b = mrdis.hip.surface_hist(flags, 3), mrdis.hip.surface_hist(flags, 3)
    assert torch.equal(a, b)
    before = mrdis.hip.launch_counts()
    mrdis.edt3d_sq(s['lab'][:1] > 0), mrdis.edt3d_sq(s['lab'] > 0)
    after = mrdis.hip.launch_counts()
    assert after['edt'] - before['edt'] == 6 and after['surfhist'] == before['surfhist'] and after['regsurf'] == before['regsurf']


# ----------------------------------------------------------------------------------------------- Run3D: predict_regions and phase score
CONTRASTS = ['T1', 'T1c', 'T2', 'T2_FLAIR']
RUN_CFG = dict(dataset_name='BraTS', contrast_list=CONTRASTS, batch_size=2, model_name='NVNet3D', init_channels=8, epochs=1, lr=1e-4,
               device='cuda:0', seed=10, predict_stride=16)
CSV_COLS = [f'{c}_{n}' for c in ('dice', 'sens', 'spec', 'hd95') for n in ('wt', 'tc', 'et')]
CSV_KEYS = [k for k in ('dice', 'sensitivity', 'specificity', 'hd95') for _ in range(3)]


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    """the tiny world of tests/test_gpu_segvol.py: 32 x 32 x 123 volumes, three served test subjects (a batch of two and a batch of one)"""
    data = data3d_volumes(n_subj=11, H=32, W=32, D=123, contrasts=CONTRASTS, seed=9)
    subj = data3d_subjects(data)
    root = tmp_path_factory.mktemp('surfdist')
    for name, part in (('train', subj[:4]), ('val', subj[4:7]), ('test', subj[7:11])):
        (root / f'fold_BraTS_3d_0_{name}_noval.txt').write_text('\n'.join(part) + '\n')
    return data, str(root), subj[8:11]


@pytest.fixture(scope='module')
def trained(mrdis, world, tmp_path_factory):
    cfg = dict(RUN_CFG, data_path=world[1], ckpt_path=str(tmp_path_factory.mktemp('ckpt')))
    store = mrdis.VolumeStore3D.from_arrays(world[0], DEV)
    mrdis.Run3D(cfg, store=store, log=lambda *a: None).train()
    return cfg, store


def read_csv(path):
    rows = open(path).read().splitlines()
    assert rows[0] == 'subj_id,' + ','.join(CSV_COLS)
    return {r.split(',')[0]: r.split(',')[1:] for r in rows[1:]}


def assert_rows_equal_scores(mrdis, rows, world, volumes, spacing=1.0):
    """every csv row = region_scores of that subject's volume against the store's seg, float for float (repr round-trips a float64)"""
    for sid, vol in volumes.items():
        seg = np.asarray(world[0][sid + '/seg'], dtype=np.float32)
        res = mrdis.region_scores(torch.from_numpy(vol[None]).to(DEV), torch.from_numpy(seg[None]).to(DEV))
        want = [float(res[k][0, i % 3]) for i, k in enumerate(CSV_KEYS)]
        got = [float(x) for x in rows[sid]]
        assert len(got) == 12 and all(g == w or (g != g and w != w) for g, w in zip(got, want)), (sid, got, want)
    return True


def test_predict_regions_writes_the_csv_and_changes_nothing_else(mrdis, world, trained, tmp_path):
    import shutil
    cfg, store = trained
    plain_dir = str(tmp_path / 'plain')
    shutil.copytree(cfg['ckpt_path'], plain_dir)
    hip = mrdis.hip
    c0 = hip.launch_counts()
    plain = mrdis.Run3D(dict(cfg, phase='predict', ckpt_path=plain_dir), store=store, log=lambda *a: None).predict()
    c1 = hip.launch_counts()
    stat = mrdis.Run3D(dict(cfg, phase='predict', predict_regions=True), store=store, log=lambda *a: None).predict()
    c2 = hip.launch_counts()
    off = {k: c1[k] - c0[k] for k in c0}
    on = {k: c2[k] - c1[k] for k in c0}
    assert all(off[k] == 0 for k in hip.SURFDIST_FAMILIES)                              # false: not one launch of the new kernels
    assert on['regsurf'] == 2 and on['surfhist'] == 2 and on['edt'] == 4                # two batches
    assert {k: v for k, v in on.items() if k not in hip.SURFDIST_FAMILIES + ('all',)} == \
        {k: v for k, v in off.items() if k not in hip.SURFDIST_FAMILIES + ('all',)}
    assert on['all'] - off['all'] == 2 * 4
    out, out_plain = os.path.join(cfg['ckpt_path'], 'result_test'), os.path.join(plain_dir, 'result_test')
    names = [f'{s}_seg.npy' for s in world[2]] + ['predict.csv']
    assert sorted(os.listdir(out_plain)) == sorted(names) and sorted(os.listdir(out)) == sorted(names + ['predict_regions.csv'])
    for n in names:
        assert open(os.path.join(out, n), 'rb').read() == open(os.path.join(out_plain, n), 'rb').read(), n
    rows = read_csv(os.path.join(out, 'predict_regions.csv'))
    assert list(rows) == world[2]
    assert_rows_equal_scores(mrdis, rows, world, {s: np.load(os.path.join(out, f'{s}_seg.npy')) for s in world[2]})
    assert set(plain) == {'dice', 'iou', 'n'} and set(stat) == {'dice', 'iou', 'n'} | set(CSV_COLS)
    assert stat['dice'] == plain['dice'] and stat['iou'] == plain['iou']
    for i, c in enumerate(CSV_COLS):
        assert stat[c] == pytest.approx(np.mean([float(rows[s][i]) for s in world[2]]), abs=1e-12)
    with pytest.raises(ValueError):
        mrdis.Run3D(dict(cfg, phase='predict', predict_regions=True, dataset_name='ZeroDose'), store=store, log=lambda *a: None)


def test_phase_score_scores_planted_volumes_without_a_model(mrdis, world, trained):
    cfg, store = trained
    out = os.path.join(cfg['ckpt_path'], 'result_test')
    os.makedirs(out, exist_ok=True)
    segs = {s: np.asarray(world[0][s + '/seg']).astype(np.uint8) for s in world[2]}
    shifted = np.zeros_like(segs[world[2][1]])
    shifted[:, 2:, :] = segs[world[2][1]][:, :-2, :]                 # the ground truth moved by 2 along W
    planted = {world[2][0]: segs[world[2][0]], world[2][1]: shifted, world[2][2]: np.zeros_like(segs[world[2][2]])}
    for s, v in planted.items():
        np.save(os.path.join(out, f'{s}_seg.npy'), v)
    before = mrdis.hip.launch_counts()
    run = mrdis.Run3D(dict(cfg, phase='score'), store=store, log=lambda *a: None)
    assert run.model is None and run.optimizer is None
    stat = run.score()
    after = mrdis.hip.launch_counts()
    assert after['all'] - before['all'] == 2 * 4 and after['regsurf'] - before['regsurf'] == 2        # two batches, nothing but the scoring kernels
    rows = read_csv(os.path.join(out, 'predict_regions.csv'))
    assert list(rows) == world[2] and stat['n'] == 3
    assert_rows_equal_scores(mrdis, rows, world, planted)
    # against the oracle, so that the values are not all the empty-region constants
    for sid, vol in planted.items():
        seg = np.asarray(world[0][sid + '/seg'], dtype=np.float32)
        flags, counts = np_flags_counts(vol[None], seg[None], BRATS_MASKS)
        want = np_scores(counts, np_hist(flags, 3, mrdis.hip.edt_bins(32, 32, 123), rho=2), (32, 32, 123), 1.0)
        got = [float(x) for x in rows[sid]]
        for i, k in enumerate(CSV_KEYS):
            w = float(want[k][0, i % 3])
            assert got[i] == w if k == 'hd95' else abs(got[i] - w) <= 1e-15, (sid, CSV_COLS[i], got[i], w)
    first = [float(x) for x in rows[world[2][0]]]
    assert first[:3] == [1.0, 1.0, 1.0] and first[9:] == [0.0, 0.0, 0.0]                 # the ground truth itself
    second = [float(x) for x in rows[world[2][1]]]
    assert all(0 < x < 1 for x in second[:3]) and all(0 < x <= 2.0 for x in second[9:])  # moved by 2: no surface voxel is further than 2 away
    third = [float(x) for x in rows[world[2][2]]]
    assert third[:3] == [0.0, 0.0, 0.0] and third[9:] == [math.sqrt(32 ** 2 + 32 ** 2 + 123 ** 2)] * 3
    # a truncated file, a wrong dtype, a wrong shape and a missing file are refused by name
    fn = os.path.join(out, f'{world[2][1]}_seg.npy')
    good = open(fn, 'rb').read()
    for spoil in ('truncated', 'dtype', 'shape', 'missing'):
        if spoil == 'truncated':
            open(fn, 'wb').write(good[:len(good) // 2])
        elif spoil == 'dtype':
            np.save(fn, shifted.astype(np.int16))
        elif spoil == 'shape':
            np.save(fn, shifted[:, :, :-1])
        else:
            os.remove(fn)
        with pytest.raises(ValueError, match=f'{world[2][1]}_seg.npy'):
            mrdis.Run3D(dict(cfg, phase='score'), store=store, log=lambda *a: None).score()
    open(fn, 'wb').write(good)
