"""Every kernel the 3-D convolution dispatcher can reach (csrc/mrdis_conv3d.hip: mrdis_conv3d_fwd, _bwd_data, _bwd_weight; the six-product
kernels of mrdis_conv3d_s6.hip; the hybrid Winograd of mrdis_wino.hip), element by element against float64 (tests/conv_check.py), with the
launch counters proving which kernel produced the result.

One row = (entry point, options, geometry) and the counted family it must launch, with its number of launches; every other counted family
(hip.CONV3D_FAMILIES, the 3-D members of hip.KERNEL_FAMILIES and all the 2-D ones) must stay at 0.  Each row reads its inputs (x, dy, the
fused residual) from channel slices of wider NDHWC buffers (ld > C, passed with their ld, not copied) and writes into a channel slice of a
wider buffer prefilled with NaN: the neighbouring channels must still hold the same NaN bits afterwards, and no output element may stay NaN
(the float64 check fails on one).  Weight-gradient rows write into caller-owned dw / db prefilled with NaN.

Where a kernel has several instantiations (tapconv3d_kernel<KC, BN>, conv3d16_kernel<KC>, wgrad3d_kernel<J>, wgrad3d16_kernel<CW>), a row
names the one it targets (`inst`) and the dispatcher rule that selects it for that geometry (`why`); test_table_covers_every_path requires
every family and every instantiation to be the target of a row.

kappa (tests/conv_check.py KAPPA): measured worst |got - ref| / (u A) per kernel and direction over all rows (profiles/conv3d_path_margins.txt,
recorded with MRDIS_DUMP_MEASURED=<dir>), times about 4."""
import pytest
import torch

import conv_check as CC
from fixtures import dump_measured

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
PAD_C = 8           # channels on each side of the input / output slices
K, PAD = 3, 1       # every 3-D convolution of the nets is 3x3x3 / pad 1 (the entry points refuse anything else)

# the families of the 3-D dispatcher: hip.CONV3D_FAMILIES and the three 3-D entries of hip.KERNEL_FAMILIES ('wino_spade' counts the hybrid 3-D
# Winograd forward / data gradient, mrdis_run_wino3d)
KERNEL_FAMILIES_3D = ('wino_spade', 'split6_c3d', 'split6_w3d')
INSTANTIATIONS = ('direct3d<4,32>', 'direct3d<4,64>', 'direct3d<8,32>', 'direct3d<8,64>',
                  'c3d16<4>', 'c3d16<8>', 'c3d16<16>', 'c3d16<32>',
                  'wgrad3d<1>', 'wgrad3d<2>', 'wgrad3d<4>', 'wgrad3d<7>', 'wgrad3d<8>', 'wgrad3d<9>',
                  'wgrad3d16<4>', 'wgrad3d16<8>', 'wgrad3d16<16>')
KAPPA = CC.KAPPA


def R(rid, op, geom, expect, opts=None, inst=None, why=None, bias=True, res=False, in_pad=PAD_C, counts=None, launches=None, kname=None):
    """geom = (N, Ci, Co, D, H, W, stride) of the layer (k = 3, pad = 1); expect = the counted family that must launch, `counts` times
    (default once); launches = the library's launches for the call ('all'); in_pad = channels right of the input slice (left: PAD_C);
    inst / why = the instantiation the row targets and the dispatcher rule that picks it; kname = the KAPPA key (default: expect)"""
    counts = counts if counts is not None else {expect: 1}
    return pytest.param(dict(op=op, geom=geom, expect=expect, opts=opts or {}, inst=inst, why=why, bias=bias, res=res, in_pad=in_pad,
                             counts=counts, launches=launches, kname=kname or expect), id=rid)


W0 = {'wino': 0}          # no Winograd: the size policy cannot take the row
W2 = {'wino': 2}          # Winograd wherever it applies
S6 = (4, 16, 16, 33, 33, 33, 1)          # the six-product gate: >= 512 boxes of 4x8x16 and >= 32768 voxels per sample; ragged in D, H and W
ROWS = [
    # ---------------------------------------------------------------- forward (mrdis_conv3d_fwd)
    R('split6_c3d fwd ragged residual', 'fwd', S6, 'split6_c3d', res=True),
    R('c3d16 fwd 4 -> 16 conv1a', 'fwd', (2, 4, 16, 6, 10, 12, 1), 'c3d16', inst='c3d16<4>', why='Cout <= 16, Cin <= 32, vec_in: KC16 = 4 for Cin <= 4'),
    R('c3d16 fwd 8 -> 8', 'fwd', (2, 8, 8, 5, 7, 9, 1), 'c3d16', inst='c3d16<8>', why='KC16 = 8 for 4 < Cin <= 8'),
    R('c3d16 fwd 16 -> 16 below the split6 gate', 'fwd', (1, 16, 16, 9, 9, 9, 1), 'c3d16', res=True, inst='c3d16<16>',
      why='16 -> 16 on 8 boxes: the six-product kernel declines (< 512 boxes); KC16 = 16'),
    R('c3d16 fwd 16 -> 16 split6=0', 'fwd', (1, 16, 16, 7, 8, 10, 1), 'c3d16', {'split6': 0}, inst='c3d16<16>', why='split6 = 0 turns the six-product kernel off'),
    R('c3d16 fwd 32 -> 16 vconv1', 'fwd', (1, 32, 16, 6, 8, 10, 1), 'c3d16', inst='c3d16<32>', why='KC16 = 32 for 16 < Cin <= 32'),
    R('c3d16 fwd cout tail 12', 'fwd', (2, 16, 12, 5, 6, 7, 1), 'c3d16', bias=False),
    R('c3d16 fwd cout 10', 'fwd', (1, 8, 10, 4, 5, 6, 1), 'c3d16'),
    R('c3d16 fwd s2 odd', 'fwd', (1, 4, 16, 7, 9, 11, 2), 'c3d16'),
    R('c3d16 fwd persistent walk', 'fwd', (2, 8, 8, 32, 48, 64, 1), 'c3d16'),         # 1536 boxes on <= 768 workgroups: the next box in flight
    R('direct3d fwd 4 -> 32', 'fwd', (2, 4, 32, 5, 6, 7, 1), 'direct3d', inst='direct3d<4,32>', why='Cout > 16: KC = 4 for Cin <= 4, BN = 32 for Cout <= 32'),
    R('direct3d fwd 24 -> 32', 'fwd', (1, 24, 32, 5, 7, 9, 1), 'direct3d', inst='direct3d<8,32>', why='KC = 8 for Cin > 4, BN = 32 for Cout <= 32'),
    R('direct3d fwd 32 -> 72 on 256 tiles', 'fwd', (1, 32, 72, 8, 32, 64, 1), 'direct3d', W0, inst='direct3d<8,64>',
      why='Cout > 32 on >= 256 (position box, 64-cout) tiles: BN = 64; KC = 8'),
    R('direct3d fwd 4 -> 40 forced BN 64', 'fwd', (1, 4, 40, 5, 6, 7, 1), 'direct3d', {'debug_kc3': 4, 'debug_bn3': 64}, inst='direct3d<4,64>',
      why='debug_bn3 = 64 forces BN = 64; KC = 4 (Cin <= 4, debug_kc3 = 4)'),
    R('direct3d fwd Ci 6 scalar loads cout 10', 'fwd', (2, 6, 10, 5, 6, 7, 1), 'direct3d', inst='direct3d<8,32>',
      why='Cin % 4 != 0: vec_in false, so not c3d16 (needs vec_in) although Cout <= 16; Cout % 4 != 0: vec_w false'),
    R('direct3d fwd input ld % 4 != 0', 'fwd', (1, 8, 16, 5, 6, 7, 1), 'direct3d', in_pad=9),        # ld = 25: vec_in false, c3d16 declines
    R('direct3d fwd no bias residual slice cout tail', 'fwd', (2, 8, 20, 4, 5, 6, 1), 'direct3d', bias=False, res=True),
    R('direct3d fwd s2 odd', 'fwd', (1, 16, 32, 7, 9, 11, 2), 'direct3d'),
    R('direct3d fwd s2 D 1', 'fwd', (2, 16, 24, 1, 6, 7, 2), 'direct3d', bias=False),
    R('direct3d fwd 1x1x1 volume', 'fwd', (2, 32, 32, 1, 1, 1, 1), 'direct3d', res=True),
    R('wino_spade fwd CG 1 D 1 odd', 'fwd', (2, 16, 24, 1, 7, 9, 1), 'wino_spade', W2, res=True),
    R('wino_spade fwd CG 2 cout tail', 'fwd', (1, 24, 40, 3, 9, 11, 1), 'wino_spade', W2, res=True),
    R('wino declines Ci % 4 -> direct3d', 'fwd', (1, 10, 24, 3, 5, 7, 1), 'direct3d', W2),
    # ---------------------------------------------------------------- data gradient (mrdis_conv3d_bwd_data: the kernel's Cin is the layer's Co)
    R('split6_c3d dgrad', 'dgrad', S6, 'split6_c3d'),
    R('c3d16 dgrad of 16 -> 32', 'dgrad', (1, 16, 32, 6, 8, 10, 1), 'c3d16', inst='c3d16<32>', why='32 in -> 16 out: KC16 = 32'),
    R('direct3d dgrad of 32 -> 64', 'dgrad', (1, 32, 64, 5, 6, 7, 1), 'direct3d', W0, inst='direct3d<8,32>', why='64 in -> 32 out: KC = 8, BN = 32'),
    R('direct3d dgrad Ci 6 vec_w off', 'dgrad', (1, 6, 40, 4, 5, 6, 1), 'direct3d', W0),          # 40 in (> 32: not c3d16) -> 6 out: scalar filter loads
    R('direct3d dgrad dy ld % 4 != 0', 'dgrad', (1, 16, 24, 4, 5, 6, 1), 'direct3d', in_pad=9),    # ld = 41: vec_in false, c3d16 declines
    R('wino_spade dgrad flip', 'dgrad', (1, 24, 40, 3, 9, 11, 1), 'wino_spade', W2),
    # stride 2: one launch per non-empty output-parity class (1, 2, 4 or 8 taps); with D = 1 the four odd-depth classes are empty
    R('dgrad s2 ds1 16 <- 32 odd', 'dgrad', (1, 16, 32, 7, 9, 11, 2), 'c3d16', counts={'c3d16': 8}, launches=8),
    R('direct3d_s2 dgrad odd', 'dgrad', (1, 32, 64, 5, 7, 9, 2), 'direct3d', counts={'direct3d': 8}, launches=8, kname='direct3d_s2'),
    R('direct3d_s2 dgrad D 1', 'dgrad', (2, 24, 32, 1, 9, 11, 2), 'direct3d', counts={'direct3d': 4}, launches=4, kname='direct3d_s2'),
    # ---------------------------------------------------------------- weight gradient (mrdis_conv3d_bwd_weight; a kernel + its reduction)
    R('wino_wgrad3d 32 -> 64', 'wgrad', (1, 32, 64, 3, 9, 11, 1), 'wino_wgrad3d', W2, counts={'wino_wgrad3d': 3}, launches=6),
    R('wino_wgrad3d 64 -> 32 no bias', 'wgrad', (2, 64, 32, 2, 6, 10, 1), 'wino_wgrad3d', W2, bias=False, counts={'wino_wgrad3d': 3}),
    R('wino_wgrad3d 64 -> 64', 'wgrad', (1, 64, 64, 2, 5, 7, 1), 'wino_wgrad3d', W2, counts={'wino_wgrad3d': 3}),
    R('split6_w3d 16 -> 16', 'wgrad', S6, 'split6_w3d', W0, launches=2),
    R('split6_w3d 32 -> 16 slices', 'wgrad', (4, 32, 16, 33, 33, 33, 1), 'split6_w3d', W0),
    R('wgrad3d16 4 -> 16', 'wgrad', (2, 4, 16, 6, 10, 12, 1), 'wgrad3d16', W0, inst='wgrad3d16<4>',
      why='stride 1, Ci, Co % 4 == 0 and each <= 16 or a multiple of 16 (plan_wgrad3d16): CW = 4 for Ci <= 4', launches=2),
    R('wgrad3d16 8 -> 8', 'wgrad', (2, 8, 8, 5, 7, 9, 1), 'wgrad3d16', W0, inst='wgrad3d16<8>', why='CW = 8 for 4 < Ci <= 8'),
    R('wgrad3d16 grid-stride walk', 'wgrad', (2, 4, 16, 16, 48, 48, 1), 'wgrad3d16', W0),        # 576 boxes on 512 split-K workgroups
    R('wgrad3d16 32 -> 32 channel slices', 'wgrad', (1, 32, 32, 5, 6, 7, 1), 'wgrad3d16', {**W0, 'split6': 0}),
    R('wgrad3d16 16 -> 48 split6=0', 'wgrad', (1, 16, 48, 5, 6, 7, 1), 'wgrad3d16', {**W0, 'split6': 0}, bias=False, inst='wgrad3d16<16>',
      why='CW = 16 for Ci >= 16; split6 = 0 keeps the six-product kernel off'),
    R('wgrad3d J9 Ci 40', 'wgrad', (1, 40, 24, 4, 5, 6, 1), 'wgrad3d', W0, inst='wgrad3d<9>',
      why='Ci = 40 (> 16, not a multiple of 16) misses plan_wgrad3d16; stride 1, Ci >= 32: CW = 32, J = 9'),
    R('wgrad3d J9 split-K walk', 'wgrad', (2, 40, 24, 8, 24, 32, 1), 'wgrad3d', W0),             # 192 position tiles on 86 splits
    R('wgrad3d J7 Ci 12', 'wgrad', (1, 12, 24, 4, 5, 6, 1), 'wgrad3d', W0, inst='wgrad3d<7>',
      why='Co = 24 (> 16, not a multiple of 16) misses plan_wgrad3d16; Ci = 12: CW = 16, two taps per sub-tile, J = 7'),
    R('wgrad3d J7 CW 8 Ci 6', 'wgrad', (1, 6, 8, 4, 5, 6, 1), 'wgrad3d', W0, bias=False, inst='wgrad3d<7>',
      why='Ci % 4 != 0 misses plan_wgrad3d16 and turns vec_x off; CW = 8, four taps per sub-tile, J = 7'),
    R('wgrad3d J4 Ci 3', 'wgrad', (2, 3, 16, 4, 5, 6, 1), 'wgrad3d', W0, inst='wgrad3d<4>', why='Ci % 4 != 0; CW = 4, eight taps per sub-tile, J = 4'),
    R('wgrad3d s2 J8 Ci 32', 'wgrad', (1, 32, 24, 5, 7, 9, 2), 'wgrad3d', W0, inst='wgrad3d<8>', why='stride 2 (eight parity groups of 8 slots): CW = 32, J = 8'),
    R('wgrad3d s2 J4 Ci 16', 'wgrad', (1, 16, 32, 7, 9, 11, 2), 'wgrad3d', W0, inst='wgrad3d<4>', why='stride 2: CW = 16, J = 8 / 2 = 4'),
    R('wgrad3d s2 J2 Ci 8', 'wgrad', (2, 8, 16, 5, 6, 7, 2), 'wgrad3d', W0, bias=False, inst='wgrad3d<2>', why='stride 2: CW = 8, J = 8 / 4 = 2'),
    R('wgrad3d s2 J1 Ci 4', 'wgrad', (2, 4, 8, 6, 7, 5, 2), 'wgrad3d', W0, inst='wgrad3d<1>', why='stride 2: CW = 4, J = 8 / 8 = 1', launches=2),
    R('wgrad3d cout 10 vec_dy off', 'wgrad', (1, 16, 10, 4, 5, 6, 1), 'wgrad3d', W0, inst='wgrad3d<7>',
      why='Co % 4 != 0 misses plan_wgrad3d16 and turns vec_dy off; Ci = 16: CW = 16, J = 7'),
]


@pytest.fixture(autouse=True)
def _cpu_threads():
    """the float64 references on at most 16 CPU threads"""
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    yield
    torch.set_num_threads(n)


def rnd(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def in_slice(t, seed, right=PAD_C):
    """t (N, C, D, H, W) as a channel slice (ld = C + PAD_C + right) of a wider NDHWC device buffer whose other channels hold random data"""
    N, C, D, H, W = t.shape
    wide = torch.cat([rnd((N, PAD_C, D, H, W), seed), t, rnd((N, right, D, H, W), seed + 1)], 1)
    wide = wide.permute(0, 2, 3, 4, 1).contiguous().to(DEV).permute(0, 4, 1, 2, 3)
    return wide[:, PAD_C:PAD_C + C]


def out_slice(N, C, D, H, W):
    """(NDHWC buffer of C + 2 PAD_C channels prefilled with NaN, the channel slice to write)"""
    buf = torch.full((N, D, H, W, C + 2 * PAD_C), float('nan'), device=DEV)
    return buf, buf.permute(0, 4, 1, 2, 3)[:, PAD_C:PAD_C + C]


def assert_neighbours_untouched(buf, C, what):
    nan = torch.full((1,), float('nan')).view(torch.int32).item()
    for side in (buf[..., :PAD_C], buf[..., PAD_C + C:]):
        assert bool((side.contiguous().view(torch.int32) == nan).all()), f'{what}: a store landed outside the output channel slice'


def tck(w):
    """(Co, Ci, 3, 3, 3) -> [27][Ci][Co] (tap = (kd * 3 + kh) * 3 + kw)"""
    return w.permute(2, 3, 4, 1, 0).reshape(27, w.shape[1], w.shape[0]).contiguous().to(DEV)


def tkc(w):
    return w.permute(2, 3, 4, 0, 1).reshape(27, w.shape[0], w.shape[1]).contiguous().to(DEV)


def run_row(hip, row, seed=0):
    """-> (results {name: (got, ref, A)}, counters since the call began)"""
    N, Ci, Co, D, H, W, st = row['geom']
    Do, Ho, Wo = ((v + 2 * PAD - K) // st + 1 for v in (D, H, W))
    op = row['op']
    x = rnd((N, Ci, D, H, W), 1 + seed)
    w = rnd((Co, Ci, K, K, K), 2 + seed, (Ci * K ** 3) ** -0.5)
    b = rnd((Co,), 3 + seed, 0.1) if row['bias'] else None
    dy = rnd((N, Co, Do, Ho, Wo), 4 + seed)
    res = {}
    if op == 'fwd':
        r = rnd((N, Co, Do, Ho, Wo), 5 + seed) if row['res'] else None
        xs, rs, wt, bd = in_slice(x, 11, row['in_pad']), None if r is None else in_slice(r, 15), tck(w), None if b is None else b.to(DEV)
        buf, out = out_slice(N, Co, Do, Ho, Wo)
        hip.launch_counts(reset=True)
        y = hip.conv3d_fwd(xs, wt, bd, K, st, PAD, residual=rs, out=out, keep_slices=True)
        c = hip.launch_counts(reset=True)
        assert y.data_ptr() == out.data_ptr()
        assert_neighbours_untouched(buf, Co, 'fwd')
        ref, A = CC.fwd_ref3d(x, w, b, st, PAD, r)
        res['y'] = (out, ref, A)
    elif op == 'dgrad':
        dys, wk = in_slice(dy, 13, row['in_pad']), tkc(w)
        buf, out = out_slice(N, Ci, D, H, W)
        hip.launch_counts(reset=True)
        dx = hip.conv3d_bwd_data(dys, wk, (N, Ci, D, H, W), K, st, PAD, out=out, keep_slices=True)
        c = hip.launch_counts(reset=True)
        assert dx.data_ptr() == out.data_ptr()
        assert_neighbours_untouched(buf, Ci, 'dgrad')
        ref, A = CC.dgrad_ref3d(dy, w, (D, H, W), st, PAD)
        res['dx'] = (out, ref, A)
    else:
        xs, dys = in_slice(x, 11, row['in_pad']), in_slice(dy, 13)
        dw = torch.full((K ** 3, Ci, Co), float('nan'), device=DEV)
        db = torch.full((Co,), float('nan'), device=DEV) if row['bias'] else None
        hip.launch_counts(reset=True)
        dw2, db2 = hip.conv3d_bwd_weight(xs, dys, K, st, PAD, row['bias'], out=(dw, db), keep_slices=True)
        c = hip.launch_counts(reset=True)
        assert dw2 is dw and db2 is db
        ref_w, A_w, ref_b, A_b = CC.wgrad_ref3d(x, dy, K, st, PAD)
        res['dw'] = (dw.reshape(K, K, K, Ci, Co).permute(4, 3, 0, 1, 2), ref_w, A_w)
        if db is not None:
            res['db'] = (db, ref_b, A_b)
    torch.cuda.synchronize()
    return res, c


@pytest.mark.parametrize('row', ROWS)
def test_conv3d_path(mrdis, row, request):
    hip = mrdis.hip
    for name, v in row['opts'].items():
        hip.set_option(name, v)
    res, c = run_row(hip, row)
    fam = {f: n for f, n in c.items() if f not in ('all', 'zsearch')}
    assert {f: n for f, n in fam.items() if n} == row['counts'], (row['counts'], {f: n for f, n in fam.items() if n})
    if row['launches'] is not None:
        assert c['all'] == row['launches'], (row['launches'], c['all'])
    kappa = KAPPA[(row['kname'], row['op'])]
    for name, (got, ref, A) in res.items():
        r = CC.ratio(got, ref, A)
        dump_measured('conv3d_path_margins.jsonl', dict(row=request.node.callspec.id, kernel=row['kname'], op=row['op'], out=name, ratio=r, kappa=kappa))
        CC.check(got, ref, A, kappa, what=f'{row["kname"]} {row["op"]} {name}')


def test_table_covers_every_path(mrdis):
    """every 3-D family (hip.CONV3D_FAMILIES and the 3-D entries of hip.KERNEL_FAMILIES) is the expected family of a row; every instantiation of
    the multi-instantiation kernels is the named target of a row that says which dispatcher rule selects it"""
    hip = mrdis.hip
    assert set(KERNEL_FAMILIES_3D) <= set(hip.KERNEL_FAMILIES) and not set(hip.CONV3D_FAMILIES) & set(hip.KERNEL_FAMILIES)
    rows = [p.values[0] for p in ROWS]
    assert {r['expect'] for r in rows} == set(hip.CONV3D_FAMILIES) | set(KERNEL_FAMILIES_3D)
    named = {r['inst'] for r in rows if r['inst']}
    assert named == set(INSTANTIATIONS), (set(INSTANTIATIONS) - named, named - set(INSTANTIATIONS))
    for p in ROWS:
        r = p.values[0]
        assert (r['kname'], r['op']) in KAPPA, p.id
        assert r['expect'] in r['counts'] and set(r['counts']) <= set(hip.CONV3D_FAMILIES) | set(KERNEL_FAMILIES_3D), p.id
        assert (r['inst'] is None) == (r['why'] is None), p.id
        assert r['inst'] is None or r['inst'].startswith(r['expect'] + '<'), p.id
