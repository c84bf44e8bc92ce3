"""The GroupNorm(+ReLU) and nearest x2-upsampling entry points of csrc/mrdis_elem3d.hip (mrdis_groupnorm_relu_fwd / _bwd / _bwd_add,
mrdis_upsample2x_add_fwd / _bwd) through the C ABI (hip.load()), element by element against float64 (tests/elem3d_check.py), at the geometries where
the launch arithmetic changes: the row-chunk edges of the statistics (GN_CHUNK_ROWS), the second trip of gn_chan_kernel's lane-strided loop, the
one-row last block of both apply kernels, every width from one channel quad to 256, G = 1 and G = C, a mean 30 sigma from zero, and the
grid-stride second trip of both upsampling kernels.  Each entry point has exactly one kernel sequence, so there is no dispatch to prove.

One GroupNorm row = (N, C, D x H x W, G, relu, input mean) and runs forward, backward and backward_add, twice: on dense rows, and on channel
slices -- x, dy and add each inside a wider buffer with its own ld (8 channels on the left, 8 / 12 / 16 on the right), y and dx into a slice of a
wider buffer prefilled with NaN (8 left, 20 right) whose neighbouring channels must keep the same NaN bits while no output element stays NaN.
Every call is made twice, into fresh NaN-prefilled outputs and a NaN-prefilled workspace of exactly mrdis_groupnorm_workspace bytes, and must
return the same bits.  backward_add is held to the bits of (dx + add) rounded once in fp32 from the plain backward's dx; the upsampling kernels
to the bits of the same fp32 expression on the CPU.

kappa (tests/elem3d_check.py KAPPA): the worst measured |got - ref| / (u A) per output over all rows, times about 4
(profiles/elem3d_path_margins.txt, recorded with MRDIS_DUMP_MEASURED=<dir>; in that run every row also evaluates the same operation in plain fp32
torch on the CPU -- the yardstick)."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import elem3d_check as E3
from fixtures import dump_measured

gpu = pytest.mark.gpu
DEV = torch.device('cuda:0')
EPS = E3.EPS
MEASURING = bool(os.environ.get('MRDIS_DUMP_MEASURED'))
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'representation-disentanglement_amd', 'csrc', 'mrdis_elem3d.hip')
OK, EINVAL, EUNSUPPORTED, EWORKSPACE, EALIGN = 0, -1, -2, -3, -5          # include/mrdis.h
LPAD = 8                                                                   # channels left of every slice: 32 bytes, the 16-byte alignment holds
RPAD = dict(x=8, dy=12, add=16, out=20)                                    # channels right of it: every view of the slice run has its own ld
KAPPA = E3.KAPPA


def kap(key):
    """the committed kappa; while measuring (MRDIS_DUMP_MEASURED) a key not yet in the table is only recorded (propagated bounds then take 16)"""
    key = ('gn', key)
    if key in KAPPA:
        return KAPPA[key]
    assert MEASURING, f'no kappa committed for {key}'
    return 16.0 if key[1] in ('mean', 'var', 'sums', 'y apply') else 1e12


@pytest.fixture(autouse=True)
def _cpu_threads():
    """the float64 references on at most 16 CPU threads"""
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    yield
    torch.set_num_threads(n)


# ---------------------------------------------------------------- the launch arithmetic of the host code, recomputed from its constants
def source_constants():
    src = open(SRC).read()
    cap = re.search(r'static int ew_blocks\(long long total\) \{ long long b = \(total \+ 255\) / 256; return \(int\)\(b > (\d+) \? (\d+) :', src)
    want = re.search(r'long long want = (\d+) / \(N > 0 \? N : 1\)', src)
    unroll = [int(u) for u in re.findall(r'gn_row_blocks\(P, C, N, (\d+), &rpb\)', src)]
    lanes = re.search(r'k < nchunk; k \+= (\d+)\)', src)
    assert cap and cap.group(1) == cap.group(2) and want and len(unroll) == 2 and lanes
    return dict(chunk_rows=int(re.search(r'#define GN_CHUNK_ROWS (\d+)', src).group(1)), block_cap=int(cap.group(1)), want=int(want.group(1)),
                unroll_fwd=unroll[0], unroll_bwd=unroll[1], chan_lanes=int(lanes.group(1)))


def gn_chunks(P, k):
    """(chunks, rows of the last one)"""
    n = -(-P // k['chunk_rows'])
    return n, P - (n - 1) * k['chunk_rows']


def gn_row_blocks(P, C, N, unroll, k):
    """gn_row_blocks of the host code -> (blocks, rows per block, rows of the last block)"""
    rows_per_pass = (256 // (C // 4)) * unroll
    want = max(k['want'] // N, 1)
    r = -(-P // want)
    r = -(-r // rows_per_pass) * rows_per_pass
    nb = -(-P // r)
    return nb, r, P - (nb - 1) * r


def test_table_covers_every_edge():
    """the rows reach every edge they are there for, under the constants the source has NOW: a later change of GN_CHUNK_ROWS, of the grid target or
    of the block cap fails here instead of silently un-covering an edge"""
    k = source_constants()
    rows = [(r, r['dhw'][0] * r['dhw'][1] * r['dhw'][2]) for r in E3.GN_ROWS]
    chunks = [gn_chunks(P, k) for _, P in rows]
    assert any(n == 1 for n, _ in chunks), 'no row with a single chunk'
    assert any(n == 1 and last == k['chunk_rows'] for n, last in chunks), 'no row whose only chunk is full'
    assert any(n == 1 and last == k['chunk_rows'] - 1 for n, last in chunks), 'no row one short of a full chunk'
    assert any(n > 1 and last == 1 for n, last in chunks), 'no row with a one-row last chunk'
    assert any(n > k['chan_lanes'] for n, _ in chunks), "no row takes gn_chan_kernel's loop into a second trip"
    for unroll in (k['unroll_fwd'], k['unroll_bwd']):
        assert any(nb > 1 and last == 1 for r, P in rows for nb, _, last in [gn_row_blocks(P, r['C'], r['N'], unroll, k)]), f'no one-row last block at unroll {unroll}'
    assert any(gn_row_blocks(P, r['C'], r['N'], k['unroll_fwd'], k)[0] > 1 and r['N'] > 1 and k['want'] % r['N'] for r, P in rows), 'no ragged split of the grid over N'
    rl = {256 // (r['C'] // 4) for r, _ in rows}
    assert {1, 2, 4, 256} <= rl, rl
    assert any(r['G'] == 1 for r, _ in rows) and any(r['G'] == r['C'] for r, _ in rows) and any(r['G'] == 2 and r['C'] // r['G'] >= 32 for r, _ in rows)
    assert any(not r['relu'] for r, _ in rows) and any(abs(r['mean']) >= 30 for r, _ in rows) and any(P == 1 for _, P in rows)
    cap = k['block_cap'] * 256
    quads = lambda g: g[0] * g[2] * g[3] * g[4] * (g[1] // 4)
    assert any(8 * quads(u['geom']) > cap and 'fwd_skip' in u['what'] for u in E3.UP_ROWS), 'no upsampling forward over the block cap'
    assert any(quads(u['geom']) > cap and 'bwd' in u['what'] for u in E3.UP_ROWS), 'no upsampling backward over the block cap'
    assert any(1 in u['geom'][2:] for u in E3.UP_ROWS) and any(u['geom'][1] == 4 for u in E3.UP_ROWS)


# ---------------------------------------------------------------- device views
def rows_of(t):
    """(N, C, D, H, W) -> the (N, P, C) row matrix"""
    N, C = t.shape[:2]
    r = t.reshape(N, C, -1).permute(0, 2, 1)
    return torch.empty(r.shape, dtype=t.dtype).copy_(r)          # (a fresh buffer: canonical strides even where P is 1)


def view_in(t, rpad, seed):
    """t (N, C, D, H, W) as a device view (N, P, C) inside a buffer of LPAD + C + rpad channels (rpad = None: dense)"""
    r = rows_of(t)
    if rpad is None:
        return r.to(DEV)
    N, P, C = r.shape
    buf = torch.cat([E3.rnd((N, P, LPAD), seed), r, E3.rnd((N, P, rpad), seed + 1)], 2).to(DEV)
    return buf[..., LPAD:LPAD + C]


def view_out(N, P, C, rpad):
    buf = torch.full((N, P, C + (LPAD + rpad if rpad is not None else 0)), float('nan'), device=DEV)
    return buf, (buf if rpad is None else buf[..., LPAD:LPAD + C])


def pl(v):
    """(pointer, leading dimension) of a view made by view_in / view_out"""
    return v.data_ptr(), v.stride(1)


def host(v, shape):
    """the (N, P, C) view's values as (N, C, D, H, W) fp32 on the host"""
    return v.detach().cpu().permute(0, 2, 1).reshape(shape).contiguous()


NAN_BITS = torch.full((1,), float('nan')).view(torch.int32).item()


def untouched(buf, C, rpad, what):
    if rpad is None:
        return
    for side in (buf[..., :LPAD], buf[..., LPAD + C:]):
        assert bool((side.contiguous().view(torch.int32) == NAN_BITS).all()), f'{what}: a store landed outside the output channel slice'


def all_nan_bits(t, what):
    assert bool((t.contiguous().view(torch.int32) == NAN_BITS).all()), f'{what}: a refused call wrote'


def f32dev(t):
    return t.float().to(DEV).contiguous()


def nan_workspace(nbytes):
    """exactly nbytes of 0xff: NaN whether read as float or as double"""
    return torch.full((max(int(nbytes), 16),), 255, dtype=torch.uint8, device=DEV)


def ok(rc, what):
    assert rc == OK, f'{what}: error {rc}'


# ---------------------------------------------------------------- GroupNorm
def gn_calls(lib, st, row, v, rpad_out):
    """forward, backward, backward_add on the views v -> the outputs on the host (y, dx, dx_add as (N, C, D, H, W); statistics and sums flat)"""
    N, C, G, relu = row['N'], row['C'], row['G'], row['relu']
    P = row['dhw'][0] * row['dhw'][1] * row['dhw'][2]
    shape = (N, C) + row['dhw']
    nb = lib.mrdis_groupnorm_workspace(N, P, C, G)
    assert nb > 0
    ybuf, y = view_out(N, P, C, rpad_out)
    mean = torch.full((N * G,), float('nan'), device=DEV); rstd = torch.full((N * G,), float('nan'), device=DEV)
    ws = nan_workspace(nb)
    ok(lib.mrdis_groupnorm_relu_fwd(*pl(v['x']), *pl(y), v['gamma'].data_ptr(), v['beta'].data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                    ws.data_ptr(), nb, N, P, C, G, EPS, relu, st), 'groupnorm_relu_fwd')
    out = dict(mean=mean.cpu(), rstd=rstd.cpu())
    bufs = [(ybuf, 'y')]
    for name, add in (('', None), ('_add', v['add'])):
        dxbuf, dx = view_out(N, P, C, rpad_out)
        dg = torch.full((C,), float('nan'), device=DEV); db = torch.full((C,), float('nan'), device=DEV)
        ws = nan_workspace(nb)
        if add is None:
            ok(lib.mrdis_groupnorm_relu_bwd(*pl(v['dy']), *pl(v['x']), v['gamma'].data_ptr(), v['beta'].data_ptr(), mean.data_ptr(), rstd.data_ptr(), *pl(dx),
                                            dg.data_ptr(), db.data_ptr(), ws.data_ptr(), nb, N, P, C, G, relu, st), 'groupnorm_relu_bwd')
        else:
            ok(lib.mrdis_groupnorm_relu_bwd_add(*pl(v['dy']), *pl(v['x']), v['gamma'].data_ptr(), v['beta'].data_ptr(), mean.data_ptr(), rstd.data_ptr(), *pl(dx),
                                                dg.data_ptr(), db.data_ptr(), *pl(add), ws.data_ptr(), nb, N, P, C, G, relu, st), 'groupnorm_relu_bwd_add')
        out.update({'dx' + name: host(dx, shape), 'dgamma' + name: dg.cpu(), 'dbeta' + name: db.cpu()})
        bufs.append((dxbuf, 'dx' + name))
    out['y'] = host(y, shape)
    for b, what in bufs:
        untouched(b, C, rpad_out, what)
    for name, t in out.items():
        assert not bool(torch.isnan(t).any()), f'{name}: an element was left unwritten (or is NaN)'
    return out


def gn_yardstick(inp, row, got, mask):
    """the same operations in plain fp32 torch on the CPU (measuring runs only)"""
    x, dy, gamma, beta = inp['x'], inp['dy'], inp['gamma'], inp['beta']
    N, C, G, relu = row['N'], row['C'], row['G'], row['relu']
    cg = C // G
    xg = x.reshape(N * G, -1)
    m32 = got['mean'].reshape(N, G, 1).expand(N, G, cg).reshape(N, C, 1, 1, 1); r32 = got['rstd'].reshape(N, G, 1).expand(N, G, cg).reshape(N, C, 1, 1, 1)
    g5, b5 = gamma.view(1, C, 1, 1, 1), beta.view(1, C, 1, 1, 1)
    xh = (x - m32) * r32
    act = (lambda t: t.clamp_min(0)) if relu else (lambda t: t)
    y = F.group_norm(x, G, gamma, beta, EPS)
    dz = dy * mask if relu else dy
    S1, S2 = dz.sum((2, 3, 4)), (dz * xh).sum((2, 3, 4))                       # (N, C)
    m = float(xg.shape[1])
    c1 = ((S1 * gamma).reshape(N, G, cg).sum(2) / m).reshape(N, G, 1).expand(N, G, cg).reshape(N, C, 1, 1, 1)
    c2 = ((S2 * gamma).reshape(N, G, cg).sum(2) / m).reshape(N, G, 1).expand(N, G, cg).reshape(N, C, 1, 1, 1)
    return {'mean': xg.mean(1), 'var': xg.var(1, unbiased=False), 'y apply': act(xh * g5 + b5), 'y': act(y), 'dbeta': S1.sum(0), 'dgamma': S2.sum(0),
            'dx': r32 * (dz * g5 - c1 - xh * c2)}


def run_gn(hip, row, sliced):
    lib, st = hip.load(), hip._stream()
    inp = E3.gn_inputs(row)
    rp = (lambda n: RPAD[n]) if sliced else (lambda n: None)
    v = dict(x=view_in(inp['x'], rp('x'), 91), dy=view_in(inp['dy'], rp('dy'), 93), add=view_in(inp['add'], rp('add'), 95),
             gamma=f32dev(inp['gamma']), beta=f32dev(inp['beta']))
    if sliced:
        assert len({pl(v[n])[1] for n in ('x', 'dy', 'add')} | {row['C'] + LPAD + RPAD['out']}) == 4
    got = gn_calls(lib, st, row, v, rp('out'))
    again = gn_calls(lib, st, row, v, rp('out'))
    for name in got:
        E3.assert_same_bits(got[name], again[name], f'{name}: second call')
    # backward_add: the bits of (dx + add) rounded once, the sums those of the plain call
    E3.assert_same_bits(got['dx_add'], got['dx'] + inp['add'], 'dx_add = fl(dx + add)')
    E3.assert_same_bits(got['dgamma_add'], got['dgamma'], 'dgamma of backward_add'); E3.assert_same_bits(got['dbeta_add'], got['dbeta'], 'dbeta of backward_add')
    x, dy, gamma, beta, G, relu = inp['x'], inp['dy'], inp['gamma'], inp['beta'], row['G'], row['relu']
    mean, rstd = got['mean'], got['rstd']
    res = []          # (output, got, ref, A, extra)
    s = E3.gn_stats_ref(x, G, EPS)
    res.append(('mean', mean, *s['mean'], None))
    res.append(('var', E3.var_from_rstd(rstd, EPS), *s['var'], E3.rstd_rounding(s['var'][0], EPS)))
    ref, A, _ = E3.gn_apply_ref(x, mean, rstd, gamma, beta, relu)
    res.append(('y apply', got['y'], ref, A, None))
    ref, A, _ = E3.gn_apply_ref(x, s['mean'][0], s['rstd'], gamma, beta, relu)
    res.append(('y', got['y'], ref, A, E3.gn_stats_propagated(x, s, gamma, kap('mean'), kap('var'), EPS)))
    mask = got['y'] > 0
    b = E3.gn_bwd_ref(dy, x, gamma, beta, mean, rstd, G, relu, mask=mask, k_apply=kap('y apply'), k_sum=kap('sums'))
    for name in ('dbeta', 'dgamma', 'dx'):
        res.append((name, got[name], *b[name]))
    yard = gn_yardstick(inp, row, got, mask) if MEASURING else {}
    return res, b, yard


@gpu
@pytest.mark.parametrize('layout', ['dense', 'slice'])
@pytest.mark.parametrize('row', [pytest.param(r, id=r['id']) for r in E3.GN_ROWS])
def test_groupnorm_path(mrdis, row, layout, request):
    res, b, yard = run_gn(mrdis.hip, row, layout == 'slice')
    failures = []
    for name, got, ref, A, extra in res:
        rec = dict(row=request.node.callspec.id, family='gn', out=name, ratio=E3.ratio(got, ref, A, 0.0, extra), kappa=KAPPA.get(('gn', name)), share=b['share'])
        if name in yard:
            rec['yardstick'] = E3.ratio(yard[name], ref, A, 0.0, extra)
        if extra is not None and MEASURING:          # how much of `extra` the result uses
            e, err = extra.double().cpu(), (got.detach().double().cpu() - ref).abs()
            rec['extra_use'] = float((err[e > 0] / e[e > 0]).max().clamp_min(0)) if bool((e > 0).any()) else 0.0
        dump_measured('elem3d_path_margins.jsonl', rec)
        try:
            E3.check(got, ref, A, kap(name), 0.0, extra, what=f'gn {name}')
        except AssertionError as e:          # every output of the row is looked at before the row fails
            failures.append(str(e))
    # conditions of the row, not tolerances: few elements sit on the ReLU's edge, and away from it the backward's mask is the forward's
    assert b['share'] <= E3.AMBIGUOUS_CAP, f"{b['share']:.2e} of the elements are within the forward bound of the ReLU's edge"
    assert b['mask_disagree'] == 0, f"{b['mask_disagree']} elements away from the ReLU's edge: stored y > 0 disagrees with float64"
    assert not failures, '\n'.join(failures)


# ---------------------------------------------------------------- nearest x2 upsampling
def ndhwc_dev(t):
    """(N, C, D, H, W) on the host -> contiguous (N, D, H, W, C) on the device"""
    return t.permute(0, 2, 3, 4, 1).contiguous().to(DEV)


def ncdhw_host(t):
    return t.cpu().permute(0, 4, 1, 2, 3)


def no_nan(t, what):
    assert not bool(torch.isnan(t).any()), f'{what}: an element was left unwritten'


@gpu
@pytest.mark.parametrize('row', [pytest.param(r, id=r['id']) for r in E3.UP_ROWS])
def test_upsample2x_path(mrdis, row):
    hip = mrdis.hip
    lib, st = hip.load(), hip._stream()
    N, C, D, H, W = row['geom']
    for what in row['what']:
        if what in ('fwd', 'fwd_skip'):
            x = E3.data((N, C, D, H, W), 1)
            skip = E3.data((N, C, 2 * D, 2 * H, 2 * W), 2) if what == 'fwd_skip' else None
            xd, sd = ndhwc_dev(x), (None if skip is None else ndhwc_dev(skip))
            ys = []
            for _ in range(2):
                y = torch.full((N, 2 * D, 2 * H, 2 * W, C), float('nan'), device=DEV)
                ok(lib.mrdis_upsample2x_add_fwd(xd.data_ptr(), None if sd is None else sd.data_ptr(), y.data_ptr(), N, D, H, W, C, st), 'upsample2x_add_fwd')
                ys.append(ncdhw_host(y))
            no_nan(ys[0], what)
            E3.assert_same_bits(ys[0], E3.up2_ref(x, skip), f'{what}: x[d/2, h/2, w/2] (+ skip) in fp32')
            E3.assert_same_bits(ys[1], ys[0], f'{what}: second call')
        else:
            shape = (N, 2 * D, 2 * H, 2 * W, C)
            if row['ints']:          # integers in [-8, 8]: every partial sum is exact, so the reference is a reshape-and-sum in any order
                dy = torch.randint(-8, 9, shape, generator=torch.Generator().manual_seed(7), dtype=torch.int8).float()
                want = dy.view(N, D, 2, H, 2, W, 2, C).sum((2, 4, 6)).permute(0, 4, 1, 2, 3)
                dyd = dy.to(DEV)
                del dy
            else:
                dy = E3.data((N, C, 2 * D, 2 * H, 2 * W), 3)
                want = E3.up2_bwd_ref(dy)
                dyd = ndhwc_dev(dy)
            dxs = []
            for _ in range(2):
                dx = torch.full((N, D, H, W, C), float('nan'), device=DEV)
                ok(lib.mrdis_upsample2x_bwd(dyd.data_ptr(), dx.data_ptr(), N, D, H, W, C, st), 'upsample2x_bwd')
                dxs.append(ncdhw_host(dx))
            no_nan(dxs[0], what)
            E3.assert_same_bits(dxs[0], want, 'bwd: the 8 children summed in order (depth, height, width) in fp32')
            E3.assert_same_bits(dxs[1], dxs[0], 'bwd: second call')


# ---------------------------------------------------------------- refusals
def gn_refusal(hip, entry, want, N=2, P=40, C=16, G=8, ldx=None, ldout=None, lddy=None, ldadd=None, offset=None, ws_short=0, null=None):
    """one refused GroupNorm call: the exact code, outputs that keep their NaN bits, no launch.  Every buffer is as large as the call would need if it
    were accepted (N, P at least 1 for the sizes), so nothing can go out of bounds even if a check were missing"""
    lib, st = hip.load(), hip._stream()
    n_, p_ = max(N, 1), max(P, 1)
    ld = dict(x=ldx or C, out=ldout or C, dy=lddy or C, add=ldadd or C)
    dev = lambda name, fill=None: (torch.full((n_ * p_ * max(ld[name], C) + 8,), float('nan'), device=DEV) if fill is None
                                   else f32dev(E3.rnd((n_ * p_ * max(ld[name], C) + 8,), fill)))
    x, dy, add, out = dev('x', 1), dev('dy', 2), dev('add', 3), dev('out')
    gamma, beta = f32dev(E3.rnd((C,), 4)), f32dev(E3.rnd((C,), 5))
    ng = n_ * max(G, 1)
    mean, rstd = torch.full((ng,), float('nan'), device=DEV), torch.full((ng,), float('nan'), device=DEV)
    dg, db = torch.full((C,), float('nan'), device=DEV), torch.full((C,), float('nan'), device=DEV)
    if entry != 'fwd':
        mean, rstd = f32dev(E3.rnd((ng,), 6)), f32dev(E3.rnd((ng,), 7).abs() + 0.5)
    nb = lib.mrdis_groupnorm_workspace(n_, p_, C, max(G, 1))          # what the call states (less ws_short); the buffer itself is larger
    assert nb > 0
    ws = nan_workspace(nb + 4096)
    ptr = {k: t.data_ptr() for k, t in dict(x=x, dy=dy, add=add, out=out, gamma=gamma, beta=beta).items()}
    if offset:
        ptr[offset] += 4
    if null:
        ptr[null] = None
    before, all0 = hip.launch_counts(elem=True), int(lib.mrdis_launch_count(b'all'))
    if entry == 'fwd':
        rc = lib.mrdis_groupnorm_relu_fwd(ptr['x'], ld['x'], ptr['out'], ld['out'], ptr['gamma'], ptr['beta'], mean.data_ptr(), rstd.data_ptr(), ws.data_ptr(),
                                          nb - ws_short, N, P, C, G, EPS, 1, st)
    elif entry == 'bwd':
        rc = lib.mrdis_groupnorm_relu_bwd(ptr['dy'], ld['dy'], ptr['x'], ld['x'], ptr['gamma'], ptr['beta'], mean.data_ptr(), rstd.data_ptr(), ptr['out'], ld['out'],
                                          dg.data_ptr(), db.data_ptr(), ws.data_ptr(), nb - ws_short, N, P, C, G, 1, st)
    else:
        rc = lib.mrdis_groupnorm_relu_bwd_add(ptr['dy'], ld['dy'], ptr['x'], ld['x'], ptr['gamma'], ptr['beta'], mean.data_ptr(), rstd.data_ptr(), ptr['out'], ld['out'],
                                              dg.data_ptr(), db.data_ptr(), ptr['add'], ld['add'], ws.data_ptr(), nb - ws_short, N, P, C, G, 1, st)
    torch.cuda.synchronize()
    case = (entry, want, dict(N=N, P=P, C=C, G=G, ld=ld, offset=offset, ws_short=ws_short, null=null))
    assert rc == want, (rc, case)
    assert hip.launch_counts(elem=True) == before and int(lib.mrdis_launch_count(b'all')) == all0, ('a refused call launched', case)
    all_nan_bits(out, case); all_nan_bits(dg, case); all_nan_bits(db, case)
    if entry == 'fwd':
        all_nan_bits(mean, case); all_nan_bits(rstd, case)
    assert bool((ws == 255).all()), ('a refused call wrote into the workspace', case)


@gpu
def test_groupnorm_refusals(mrdis):
    hip = mrdis.hip
    entries = ('fwd', 'bwd', 'bwd_add')
    for e in entries:
        for C, G in ((24, 8), (48, 8), (6, 2), (2048, 8), (16, 3)):          # C / 4 does not divide 256 | C % 4 | C / 4 > 256 | C % G
            gn_refusal(hip, e, EUNSUPPORTED, P=4, C=C, G=G)
        gn_refusal(hip, e, EUNSUPPORTED, ldx=16 + 2)
        gn_refusal(hip, e, EUNSUPPORTED, ldout=16 - 4)
        gn_refusal(hip, e, EALIGN, offset='x')
        gn_refusal(hip, e, EALIGN, offset='out')
        gn_refusal(hip, e, EWORKSPACE, ws_short=1)
        gn_refusal(hip, e, EINVAL, N=0)
        gn_refusal(hip, e, EINVAL, P=0)
        gn_refusal(hip, e, EINVAL, null='gamma')
    for e in entries[1:]:
        gn_refusal(hip, e, EUNSUPPORTED, lddy=16 + 2)
        gn_refusal(hip, e, EUNSUPPORTED, lddy=16 - 4)
        gn_refusal(hip, e, EALIGN, offset='dy')
    gn_refusal(hip, 'bwd_add', EUNSUPPORTED, ldadd=16 + 2)
    gn_refusal(hip, 'bwd_add', EUNSUPPORTED, ldadd=16 - 4)
    gn_refusal(hip, 'bwd_add', EALIGN, offset='add')


@gpu
def test_upsample2x_refusals(mrdis):
    hip = mrdis.hip
    lib, st = hip.load(), hip._stream()
    N, D, H, W = 2, 2, 3, 2
    x = f32dev(E3.rnd((N * 8 * D * H * W * 8 + 8,), 1))          # large enough to be either operand of any case below
    cases = [(dict(C=6), EUNSUPPORTED, 0), (dict(D=0), EINVAL, 0), (dict(C=8), EALIGN, 4)]
    for kw, want, off in cases:
        g = dict(N=N, D=D, H=H, W=W, C=8); g.update(kw)
        out = torch.full((N * 8 * D * H * W * 8 + 8,), float('nan'), device=DEV)
        before, all0 = hip.launch_counts(elem=True), int(lib.mrdis_launch_count(b'all'))
        rc_f = lib.mrdis_upsample2x_add_fwd(x.data_ptr(), x.data_ptr(), out.data_ptr() + off, g['N'], g['D'], g['H'], g['W'], g['C'], st)
        rc_b = lib.mrdis_upsample2x_bwd(x.data_ptr(), out.data_ptr() + off, g['N'], g['D'], g['H'], g['W'], g['C'], st)
        torch.cuda.synchronize()
        assert (rc_f, rc_b) == (want, want), (rc_f, rc_b, want, kw)
        assert hip.launch_counts(elem=True) == before and int(lib.mrdis_launch_count(b'all')) == all0, ('a refused call launched', kw)
        all_nan_bits(out, kw)
