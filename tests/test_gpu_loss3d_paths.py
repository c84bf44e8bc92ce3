"""Every phase of the streaming loop of csrc/mrdis_loss3d.hip (l3_stream: unrolled body, remainder, n % 4 tail) and every instantiation of its
seg_counts_kernel<C, VEC>, element by element against float64 (tests/loss3d_check.py), through the C ABI (hip.load() and ctypes: the rows choose the
pointers, the workspace size, w_l2 and the upstream gradient themselves).

One row = one geometry (loss3d_check.OBJECTIVE_ROWS / SEG_ROWS: sizes stated in L3_THREADS, L3_MAX_BLOCKS and L3_UNROLL as the source has them) and one
seed.  A row is a function of an implementation object: HipImpl runs the kernels, TorchImpl evaluates the same operation in plain torch on the CPU --
the yardstick.  tests/test_loss3d_check.py runs every row with TorchImpl (no GPU) and holds loss3d_check.KAPPA to 4 x the worst yardstick ratio; the
tests below run them with HipImpl under that table.

An objective row runs, for each (g, w_l2) of its pairs: the forward twice (same bits; sums and terms prefilled with NaN; the workspace exactly as large
as mrdis_nvnet_loss_workspace says, NaN behind it that must stay), the backward with both gradients twice (same bits), with du alone and with dv alone
(the bits of the joint call: their grids are sized by the one pair).  du / dv are the first n floats of 16-byte aligned buffers of n + 64 NaN: the 64
behind keep their bits, none in front stays NaN.  Every entry call counts 'loss3d' once and nothing else ('all': 2 launches forward, 1 backward).
terms and du are held to references formed from the sums the forward STORED, so each stage answers for its own rounding.

MRDIS_DUMP_MEASURED=<dir> records both ratios of every row (loss3d_path_margins.jsonl; profiles/loss3d_path_margins.txt)."""
import ctypes as C_
import os

import pytest
import torch

import loss3d_check as LC
from fixtures import dump_measured

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
NAN = float('nan')
MEASURING = bool(os.environ.get('MRDIS_DUMP_MEASURED'))
L3_THREADS, L3_MAX_BLOCKS, L3_UNROLL = LC.source_constants()          # read out of csrc/mrdis_loss3d.hip by regex
T, UN = L3_MAX_BLOCKS * L3_THREADS, L3_UNROLL
EINVAL, EUNSUPPORTED, EWORKSPACE, EALIGN = -1, -2, -3, -5
GUARD = 64


@pytest.fixture(autouse=True)
def _cpu_threads():
    """the float64 references on at most 16 CPU threads"""
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    yield
    torch.set_num_threads(n)


def same_bits(a, b, what):
    a, b = a.detach().contiguous(), b.detach().contiguous()
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    bad = a.view(torch.int32) != b.view(torch.int32)          # (on the tensors' own device: a 9 M-float gradient is compared where it lies)
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} of {bad.numel()} words differ in their bits'


def is_nan_bits(t, what):
    if t.dtype is torch.float64:
        nan = torch.full((1,), NAN, dtype=torch.float64).view(torch.int64).item()
        ok = t.contiguous().view(torch.int64) == nan
    else:
        nan = torch.full((1,), NAN).view(torch.int32).item()
        ok = t.contiguous().view(torch.int32) == nan
    assert bool(ok.all()), f'{what}: a store landed outside the output'


class Rec:
    """collects (output, kappa key, ratio) of one row; enforce: every output is held to its committed kappa"""

    def __init__(self, rid, enforce):
        self.rid, self.enforce, self.items = rid, enforce, []

    def __call__(self, name, key, got, ref, A):
        if self.enforce:
            assert key in LC.KAPPA, f'no kappa committed for {key}'
            r = LC.check(got, ref, A, LC.KAPPA[key], what=f'{self.rid}: {name}')
        else:
            r = LC.ratio(got, ref, A)
        self.items.append((name, key, r))


def dense(shape):
    """NCDHW-contiguous strides"""
    s, acc = [], 1
    for e in reversed(shape):
        s.append(acc); acc *= e
    return tuple(reversed(s))


def default_layout(c):
    """(shape1, strides u, strides t, shape2, strides v, strides x): both pairs dense in NCDHW order"""
    s1, s2 = c['shape1'], c['shape2']
    return (s1, dense(s1), dense(s1), s2, None if s2 is None else dense(s2), None if s2 is None else dense(s2))


# ================================================================ implementations
class TorchImpl:
    """plain torch on the CPU: the yardstick (loss3d_check.sums_t / objective_t).  Layouts do not apply: every operation is element-wise or a flat sum"""
    gpu = False

    def __init__(self):
        self._sums = {}

    def objective(self, c, g, w_l2, lay=None):
        key = c['rid']
        if key not in self._sums:
            self._sums = {key: LC.sums_t(c['u'], c['t'], c['v'], c['x'])}
        o = LC.objective_t(c['u'], c['t'], c['v'], c['x'], w_l2, g)
        return dict(o, sums=self._sums[key])

    def seg_counts(self, pred, target, logits, offset=0):
        pp, tt = (torch.sigmoid(pred) if logits else pred) > 0.5, target == 1
        return torch.stack([(pp & tt).sum(1), pp.sum(1), tt.sum(1)], -1)


def ll(values):
    return None if values is None else (C_.c_longlong * len(values))(*values)


def ptr(t):
    return None if t is None else t.data_ptr()


class HipImpl:
    """the kernels under test, through the C ABI"""
    gpu = True

    def __init__(self, m):
        self.hip, self.lib = m.hip, m.hip.load()
        self._dev = {}

    def st(self):
        return self.hip._stream()

    def call(self, fam, launches, fn, *args):
        """one accepted call and its counters: the family once, 'all' the launches, nothing else"""
        self.hip.launch_counts(reset=True)
        rc = fn(*args)
        assert rc == 0, (fn.__name__, rc)
        got = {k: n for k, n in self.hip.launch_counts(reset=True, elem=True).items() if n}
        assert got == {fam: 1, 'all': launches}, f'{fn.__name__}: counted {got}, the row expects {fam} once in {launches} launches'

    def refused(self, want, fn, *args):
        self.hip.launch_counts(reset=True)
        rc = fn(*args)
        moved = {k: n for k, n in self.hip.launch_counts(reset=True, elem=True).items() if n}
        assert rc == want and not moved, (fn.__name__, rc, want, moved)

    def dev(self, c):
        key = c['rid']
        if key not in self._dev:
            self._dev = {key: {k: (None if c[k] is None else c[k].to(DEV)) for k in ('u', 't', 'v', 'x')}}
        return self._dev[key]

    def fwd(self, d, lay, n1, n2, w_l2):
        """-> (sums, terms) on the device, of two calls with the same bits"""
        lib = self.lib
        s1, su, st_, s2, sv, sx = lay
        nb = lib.mrdis_nvnet_loss_workspace(n1, n2)
        assert nb == 32 * LC.l3_blocks(n1, n2)
        runs = []
        for _ in range(2):
            sums, terms = torch.full((4,), NAN, dtype=torch.float64, device=DEV), torch.full((3,), NAN, device=DEV)
            ws = torch.full((nb // 8 + 512,), NAN, dtype=torch.float64, device=DEV)
            self.call('loss3d', 2, lib.mrdis_nvnet_loss_fwd, ptr(d['u']), ll(su), ptr(d['t']), ll(st_), ll(s1), 5, ptr(d['v']), ll(sv), ptr(d['x']), ll(sx), ll(s2),
                      5 if s2 else 0, w_l2, sums.data_ptr(), terms.data_ptr(), ws.data_ptr(), nb, self.st())
            is_nan_bits(ws[nb // 8:], 'nvnet_loss_fwd workspace tail')
            runs.append((sums, terms))
        same_bits(runs[1][0], runs[0][0], 'sums: second call'); same_bits(runs[1][1], runs[0][1], 'terms: second call')
        return runs[0]

    def bwd(self, d, lay, n1, n2, w_l2, sums, g, need_du, need_dv):
        s1, su, st_, s2, sv, sx = lay
        du = torch.full((n1 + GUARD,), NAN, device=DEV) if need_du else None
        dv = torch.full((n2 + GUARD,), NAN, device=DEV) if need_dv else None
        self.call('loss3d', 1, self.lib.mrdis_nvnet_loss_bwd, ptr(d['u']), ll(su), ptr(d['t']), ll(st_), ll(s1), 5, ptr(d['v']), ll(sv), ptr(d['x']), ll(sx), ll(s2),
                  5 if s2 else 0, w_l2, sums.data_ptr(), g.data_ptr(), ptr(du), ptr(dv), self.st())
        for name, buf, n in (('du', du, n1), ('dv', dv, n2)):
            if buf is not None:
                assert buf.data_ptr() % 16 == 0
                is_nan_bits(buf[n:], f'{name}: the {GUARD} floats behind')
                assert not bool(torch.isnan(buf[:n]).any()), f'{name}: an element was never written'
        return (None if du is None else du[:n1]), (None if dv is None else dv[:n2])

    def objective(self, c, g, w_l2, lay=None):
        d, lay = self.dev(c), lay or default_layout(c)
        n1, n2 = c['n1'], c['n2']
        sums, terms = self.fwd(d, lay, n1, n2, w_l2)
        gd = torch.tensor([g], dtype=torch.float32, device=DEV)
        du, dv = self.bwd(d, lay, n1, n2, w_l2, sums, gd, True, n2 > 0)
        du2, dv2 = self.bwd(d, lay, n1, n2, w_l2, sums, gd, True, n2 > 0)
        same_bits(du2, du, 'du: second call')
        if n2:
            same_bits(dv2, dv, 'dv: second call')
            same_bits(self.bwd(d, lay, n1, n2, w_l2, sums, gd, True, False)[0], du, 'du alone against the joint call')
            same_bits(self.bwd(d, lay, n1, n2, w_l2, sums, gd, False, True)[1], dv, 'dv alone against the joint call')
        s = sums.cpu()
        return dict(sums=s, stored=s, terms=terms.cpu(), du=du.cpu(), dv=None if dv is None else dv.cpu())

    def seg_counts(self, pred, target, logits, offset=0):
        """-> what the call ADDED to an `out` prefilled with arange, (B, C, 3) int64"""
        B, P, C = pred.shape
        n = pred.numel()
        bufs = []
        for t in (pred, target):
            b = torch.full((n + 8,), NAN, device=DEV)
            b[offset:offset + n] = t.reshape(-1).to(DEV)
            bufs.append(b[offset:offset + n])
        assert all(b.data_ptr() % 16 == 4 * (offset % 4) for b in bufs)
        out = torch.arange(B * C * 3, dtype=torch.int32, device=DEV)
        self.call('segcounts', 1, self.lib.mrdis_seg_counts, bufs[0].data_ptr(), bufs[1].data_ptr(), out.data_ptr(), B, P, C, int(logits), self.st())
        return (out.cpu().long() - torch.arange(B * C * 3)).reshape(B, C, 3)


# ================================================================ objective rows
def row_objective(row, impl, rec):
    c = LC.objective_case(row['id'])
    sref, base = LC.sums_ref(c['u'], c['t'], c['v'], c['x']), None
    first = None
    for g, w in row['pairs']:
        tag = f' g {g} w {w}'
        o = impl.objective(c, g, w)
        if first is None:
            first = o
            rec('sums', ('fwd', 'sums'), o['sums'], *sref)
            base = LC.du_ref(c['u'], c['t'], o['stored'], 1.0)          # once per row: g scales ref and A alike
        else:          # neither g nor w_l2 enters the sums
            LC.assert_same_bits(o['sums'], first['sums'], 'sums' + tag); LC.assert_same_bits(o['stored'], first['stored'], 'stored sums' + tag)
        tr = LC.terms_ref(o['stored'], c['n2'], w)
        for i, k in enumerate(('dice', 'l2', 'obj')):
            rec(k + tag, ('fwd', k), o['terms'][i:i + 1], *tr[k])
        g32 = LC.f32(g)          # the references from the operands the kernel reads: g is an fp32 scalar on the device
        rec('du' + tag, ('bwd', 'du'), o['du'], g32 * base[0], abs(g32) * base[1])
        assert (o['dv'] is None) == (c['n2'] == 0)
        if c['n2']:
            rec('dv' + tag, ('bwd', 'dv'), o['dv'], *LC.dv_ref(c['v'], c['x'], g32, w))
            if w == 0:
                assert not bool(o['dv'].any()), 'dv with w_l2 = 0'
    if row['tmode'] == 'zeros':
        assert float(first['stored'][0]) == 0.0 and float(first['stored'][2]) == 0.0          # A0 = 0: c2 = 0, dice = 1
        assert float(first['terms'][0]) == 1.0


def row_layout(row, impl, rec):
    """the 'tail1' size as (1, 3, 5, 7, 9) and (1, 5, 5, 7, 9) under four stride sets over ONE flat buffer per tensor: the flat order is the same, so
    all four share their sums to the bit; du and dv are compared through the logical view the strides give"""
    c = dict(LC.objective_case('tail1'))
    g, w = 0.37, 0.1
    g32 = LC.f32(g)
    first = None
    for k, name in enumerate(n for n, _ in LC.layout_strides(3)):
        s1, s2 = (1, 3) + LC.LAYOUT_DHW, (1, 5) + LC.LAYOUT_DHW
        assert s1[0] * s1[1] * 315 == c['n1'] and s2[0] * s2[1] * 315 == c['n2']
        su, sv = LC.layout_strides(3)[k][1], LC.layout_strides(5)[k][1]
        st_, sx = su, sv
        if k == 3:          # an extent of 1 carries no layout: accepted
            st_, sx = (LC.LAYOUT_BATCH_STRIDE_T,) + su[1:], (LC.LAYOUT_BATCH_STRIDE_T,) + sv[1:]
        o = impl.objective(c, g, w, lay=(s1, su, st_, s2, sv, sx))
        if first is None:
            first = o
        else:
            LC.assert_same_bits(o['sums'], first['sums'], f'sums of {name} against dense: one flat buffer'); LC.assert_same_bits(o['du'], first['du'], f'du (flat) of {name}')
        rec('sums ' + name, ('fwd', 'sums'), o['sums'], *LC.sums_ref(c['u'], c['t'], c['v'], c['x']))
        view = lambda t, s, st: t.as_strided(s, st)
        ref = LC.du_ref(view(c['u'], s1, su), view(c['t'], s1, st_), o['stored'], g32)
        rec('du ' + name, ('bwd', 'du'), view(o['du'], s1, su), *ref)
        rec('dv ' + name, ('bwd', 'dv'), view(o['dv'], s2, sv), *LC.dv_ref(view(c['v'], s2, sv), view(c['x'], s2, sx), g32, w))
        if impl.gpu:          # the wrapper: du comes back in uout's strides, with the bits of the C-ABI call
            d = impl.dev(c)
            u, t, v, x = view(d['u'], s1, su), view(d['t'], s1, st_), view(d['v'], s2, sv), view(d['x'], s2, sx)
            sums, _ = impl.hip.nvnet_loss_fwd(u, t, v, x, w)
            du, dv = impl.hip.nvnet_loss_bwd(torch.tensor([g], device=DEV), sums, u, t, v, x, w)
            assert du.stride() == u.stride() and dv.stride() == v.stride() and du.shape == u.shape
            LC.assert_same_bits(sums.cpu(), o['sums'], 'wrapper sums ' + name)
            LC.assert_same_bits(du.cpu(), view(o['du'], s1, su), 'wrapper du ' + name); LC.assert_same_bits(dv.cpu(), view(o['dv'], s2, sv), 'wrapper dv ' + name)


def row_seg(row, impl, rec):
    geo = LC.seg_geometry(row)
    assert geo['vec'] == row['vec'], 'the row states the wrong instantiation'
    assert row['blocks'] is None or row['blocks'] == (geo['want'], geo['launched']), ('the row states the wrong grid', geo)
    c = LC.seg_case(row['id'])
    for logits in (True, False):
        pred = c['logits'] if logits else c['probs']
        lo, hi = LC.seg_counts_bounds(pred, c['target'], logits)
        got = impl.seg_counts(pred, c['target'], logits, row['offset'])
        bad = (got < lo) | (got > hi)
        assert not bool(bad.any()), (row['id'], 'logits' if logits else 'probabilities', bad.nonzero()[:4].tolist(), got[bad][:4].tolist(), lo[bad][:4].tolist(), hi[bad][:4].tolist())


OBJ_PARAMS = [pytest.param('objective', r, id='objective ' + r['id']) for r in LC.OBJECTIVE_ROWS]
LAYOUT_PARAMS = [pytest.param('layout', dict(id='layouts'), id='layouts of the tail1 size')]
SEG_PARAMS = [pytest.param('seg', r, id='seg_counts ' + r['id']) for r in LC.SEG_ROWS]
ALL_ROWS = OBJ_PARAMS + LAYOUT_PARAMS + SEG_PARAMS
ROW_FN = dict(objective=row_objective, layout=row_layout, seg=row_seg)


def run_row(op, row, impl, rid, enforce):
    rec = Rec(rid, enforce)
    ROW_FN[op](row, impl, rec)
    return rec.items


@pytest.mark.parametrize('op,row', ALL_ROWS)
def test_loss3d_path(mrdis, request, op, row):
    rid = request.node.callspec.id
    items = run_row(op, row, HipImpl(mrdis), rid, enforce=not MEASURING)
    if MEASURING:
        yard = {name: r for name, _, r in run_row(op, row, TorchImpl(), rid, False)}
        for name, key, r in items:
            dump_measured('loss3d_path_margins.jsonl', dict(row=rid, out=name, key=list(key), kernel=r, yardstick=yard.get(name), kappa=LC.KAPPA.get(key)))
        for name, key, r in items:
            assert key in LC.KAPPA and r <= LC.KAPPA[key], f'{rid}: {name} needs kappa {r:.2f}, committed {LC.KAPPA.get(key)}'


# ================================================================ refusals: argument checks that run before any launch; real, fully sized buffers
def test_objective_refusals_launch_nothing(mrdis):
    impl = HipImpl(mrdis)
    lib, st = impl.lib, impl.st()
    c = LC.objective_case('tail1')
    n1, n2 = c['n1'], c['n2']
    lay = default_layout(c)
    s1, su, st_, s2, sv, sx = (ll(a) for a in lay)
    big = {k: torch.zeros(c[k].numel() + 4, device=DEV) for k in ('u', 't', 'v', 'x')}          # views one float in: 4 bytes past alignment
    for k in big:
        big[k][1:1 + c[k].numel()] = c[k].to(DEV)
    d = {k: big[k][:c[k].numel()] for k in big}
    off = {k: big[k][1:1 + c[k].numel()] for k in big}
    nb = lib.mrdis_nvnet_loss_workspace(n1, n2)
    sums, terms = torch.full((4,), NAN, dtype=torch.float64, device=DEV), torch.full((3,), NAN, device=DEV)
    ws = torch.full((nb // 8,), NAN, dtype=torch.float64, device=DEV)
    g = torch.ones(1, device=DEV)
    du, dv = torch.full((n1 + GUARD,), NAN, device=DEV), torch.full((n2 + GUARD,), NAN, device=DEV)

    zsums = torch.ones(4, dtype=torch.float64, device=DEV)

    def fwd(want, u=d['u'], t=d['t'], v=d['v'], x=d['x'], nbytes=nb):
        args = (lib.mrdis_nvnet_loss_fwd, ptr(u), su, ptr(t), st_, s1, 5, ptr(v), sv, ptr(x), sx, s2, 5, 0.1, sums.data_ptr(), terms.data_ptr(), ws.data_ptr(), nbytes, st)
        impl.refused(want, *args) if want else impl.call('loss3d', 2, *args)

    def bwd(want, u=d['u'], v=d['v'], x=d['x'], du_=du, dv_=dv):
        args = (lib.mrdis_nvnet_loss_bwd, ptr(u), su, ptr(d['t']), st_, s1, 5, ptr(v), sv, ptr(x), sx, s2, 5, 0.1, zsums.data_ptr(), g.data_ptr(), ptr(du_), ptr(dv_), st)
        impl.refused(want, *args) if want else impl.call('loss3d', 1, *args)

    fwd(EALIGN, u=off['u']); fwd(EALIGN, t=off['t']); fwd(EALIGN, v=off['v']); fwd(EALIGN, x=off['x'])
    fwd(EWORKSPACE, nbytes=nb - 1)
    fwd(EINVAL, x=None)                               # vout without x
    fwd(EINVAL, v=None)                               # x without vout
    bwd(EALIGN, u=off['u']); bwd(EALIGN, du_=du[1:]); bwd(EALIGN, dv_=dv[1:])
    bwd(EINVAL, x=None)                               # vout without x
    bwd(EINVAL, v=None, x=None)                       # dv wanted without vout
    bwd(EINVAL, du_=None, dv_=None)                   # neither gradient wanted
    torch.cuda.synchronize()
    for t in (sums, terms, ws, du, dv):
        is_nan_bits(t, 'a refused call wrote')
    fwd(0); bwd(0)                                    # the control: the same arguments without an override are accepted, and write
    assert not bool(torch.isnan(sums).any()) and not bool(torch.isnan(du[:n1]).any()) and not bool(torch.isnan(dv[:n2]).any())
    is_nan_bits(du[n1:], 'du guard'); is_nan_bits(dv[n2:], 'dv guard')


def test_seg_counts_refusals_launch_nothing(mrdis):
    impl = HipImpl(mrdis)
    lib, st = impl.lib, impl.st()
    for B, C, P in ((2, 5, 4), (65536, 1, 1)):
        pred, tgt = torch.zeros(B * P * C, device=DEV), torch.zeros(B * P * C, device=DEV)
        out = torch.arange(B * C * 3, dtype=torch.int32, device=DEV)
        impl.refused(EUNSUPPORTED, lib.mrdis_seg_counts, pred.data_ptr(), tgt.data_ptr(), out.data_ptr(), B, P, C, 1, st)
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), torch.arange(B * C * 3, dtype=torch.int32))


# ================================================================ through model3d.nvnet_loss_hip
def _function_case():
    c = LC.objective_case('tail1')
    s1, s2 = (1, 3) + LC.LAYOUT_DHW, (1, 5) + LC.LAYOUT_DHW
    cl = lambda t, s: t.to(DEV).reshape(s[0], *s[2:], s[1]).permute(0, 4, 1, 2, 3)          # channels-last-3d, as the nets write it
    g = torch.Generator().manual_seed(5)
    mu, logvar = torch.randn(1, 16, generator=g).to(DEV), (0.1 * torch.randn(1, 16, generator=g)).to(DEV)
    return c, cl(c['u'], s1), cl(c['t'], s1), cl(c['v'], s2), cl(c['x'], s2), mu, logvar


def _flat(t):
    """a channels-last-3d gradient in its memory order"""
    return t.permute(0, 2, 3, 4, 1).reshape(-1).cpu()


@pytest.mark.parametrize('scale', [0.37, -1.0])
def test_function_scaled_loss_backward(mrdis, scale):
    hip = mrdis.hip
    c, u, t, v, x, mu, logvar = _function_case()
    u, v = u.detach().requires_grad_(True), v.detach().requires_grad_(True)
    hip.launch_counts(reset=True)
    loss, parts = mrdis.nvnet_loss_hip(u, v, mu, logvar, x, t)
    (scale * loss).backward()
    got = {k: n for k, n in hip.launch_counts(reset=True).items() if n and k != 'all'}
    assert got == {'loss3d': 2}, got
    sums, terms = hip.nvnet_loss_fwd(u.detach(), t, v.detach(), x, 0.1)
    assert u.grad.stride() == u.stride() and v.grad.stride() == v.stride()
    LC.check(_flat(u.grad), *LC.du_ref(c['u'], c['t'], sums.cpu(), LC.f32(scale)), LC.KAPPA[('bwd', 'du')], what=f'du of ({scale} loss).backward()')
    LC.check(_flat(v.grad), *LC.dv_ref(c['v'], c['x'], LC.f32(scale), 0.1), LC.KAPPA[('bwd', 'dv')], what=f'dv of ({scale} loss).backward()')
    tr = LC.terms_ref(sums.cpu(), c['n2'], 0.1)
    LC.check(parts['dice'].reshape(1), *tr['dice'], LC.KAPPA[('fwd', 'dice')], what='parts dice'); LC.check(parts['l2'].reshape(1), *tr['l2'], LC.KAPPA[('fwd', 'l2')], what='parts l2')


def test_function_detached_inputs_and_dice_only(mrdis):
    hip = mrdis.hip
    c, u, t, v, x, mu, logvar = _function_case()
    ur, vr = u.detach().requires_grad_(True), v.detach().requires_grad_(True)
    mrdis.nvnet_loss_hip(ur, vr, mu, logvar, x, t)[0].backward()
    # uout detached: no du, one count for the backward
    v1 = v.detach().requires_grad_(True)
    loss, _ = mrdis.nvnet_loss_hip(u.detach(), v1, mu, logvar, x, t)
    hip.launch_counts(reset=True)
    loss.backward()
    assert {k: n for k, n in hip.launch_counts(reset=True).items() if n and k != 'all'} == {'loss3d': 1}
    LC.assert_same_bits(v1.grad, vr.grad, 'dv with uout detached')
    # vout detached: no dv
    u1 = u.detach().requires_grad_(True)
    vd = v.detach()
    loss, _ = mrdis.nvnet_loss_hip(u1, vd, mu, logvar, x, t)
    hip.launch_counts(reset=True)
    loss.backward()
    assert {k: n for k, n in hip.launch_counts(reset=True).items() if n and k != 'all'} == {'loss3d': 1}
    assert vd.grad is None
    LC.assert_same_bits(u1.grad, ur.grad, 'du with vout detached')
    # the Dice-only objective
    u2 = u.detach().requires_grad_(True)
    hip.launch_counts(reset=True)
    loss, parts = mrdis.nvnet_loss_hip(u2, None, None, None, None, t)
    loss.backward()
    assert {k: n for k, n in hip.launch_counts(reset=True).items() if n and k != 'all'} == {'loss3d': 2}
    sums, _ = hip.nvnet_loss_fwd(u.detach(), t)
    tr = LC.terms_ref(sums.cpu(), 0, 0.1)
    LC.check(loss.detach().reshape(1), *tr['dice'], LC.KAPPA[('fwd', 'dice')], what='Dice-only loss')
    assert float(parts['l2']) == 0.0 and float(parts['kl']) == 0.0 and float(loss.detach()) == float(parts['dice'])
    LC.check(_flat(u2.grad), *LC.du_ref(c['u'], c['t'], sums.cpu(), 1.0), LC.KAPPA[('bwd', 'du')], what='Dice-only du')
    LC.assert_same_bits(u2.grad, ur.grad, 'Dice-only du against the full objective: the Dice sums are the same')


# ================================================================ the table against the source's constants
def test_table_covers_every_path():
    """every phase of l3_stream (body yes / no; remainder for no, some or all threads; a tail of 0, 1, 2, 3) is the named target of a row, with the
    inequality on n, T = L3_MAX_BLOCKS * L3_THREADS and U = L3_UNROLL that puts it there; every seg_counts_kernel<C, VEC> instantiation likewise.
    The inequalities are asserted against the constants read out of the source: a change of L3_MAX_BLOCKS fails the table instead of emptying a row"""
    seen = set()
    for row in LC.OBJECTIVE_ROWS:
        assert row['phases'] and row['why']
        for (launch, pair), claim in row['phases'].items():
            ph = LC.stream_phases(row['n1'] if pair == 1 else row['n2'], LC.launch_threads(row, launch))
            assert LC.phase_name(ph) == claim, (row['id'], launch, pair, ph, claim)
            seen.add(claim)
    assert {s[0] for s in seen} == {False, True} and {s[1] for s in seen} == {'zero', 'partial', 'all'} and {s[2] for s in seen} == {0, 1, 2, 3}, seen
    for combo in ((True, 'partial', 3), (True, 'zero', 0), (False, 'zero', 3), (False, 'all', 2), (False, 'partial', 1)):
        assert combo in seen, combo
    R = LC.OBJECTIVE
    for n in (R['all phases']['n1'], R['all phases']['n2']):
        nv = n // 4
        assert nv > T                                             # the cap binds: more groups than L3_MAX_BLOCKS blocks have threads
        assert (T - 1) + (UN - 1) * T < nv                        # the last thread's fourth load is in range: every thread takes the body
        assert nv <= (2 * UN - 1) * T                             # ... once
        assert UN * T < nv < UN * T + T and nv - UN * T == T // 2 + 37          # the remainder: threads 0 .. T/2 + 36, once
    assert (R['all phases']['n1'] % 4, R['all phases']['n2'] % 4) == (3, 1)
    nv = R['partial body']['n1'] // 4
    ph = LC.stream_phases(R['partial body']['n1'], T)
    assert (UN - 1) * T < nv < UN * T and ph['body'] == nv - (UN - 1) * T == 100 and ph['rem'] == T - 100 and ph['rem_max'] == UN - 1 and LC.l3_blocks(4 * nv, 0) == L3_MAX_BLOCKS
    ph = LC.stream_phases(R['body exact']['n1'], T)
    assert R['body exact']['n1'] == 4 * 2 * UN * T and (ph['body'], ph['body_max'], ph['rem'], ph['tail']) == (T, 2, 0, 0)
    for rid, small, alone in (('big u small v', 'n2', 'dv'), ('small u big v', 'n1', 'du')):
        row = R[rid]
        assert LC.launch_threads(row, 'joint') == T                                      # sized by the larger pair, capped
        ph = LC.stream_phases(row[small], T)
        assert 0 < ph['rem'] == row[small] // 4 < T // 1000 and ph['body'] == 0          # most threads idle on the small pair
        assert LC.launch_threads(row, alone) == L3_THREADS * -(-(row[small] // 4) // L3_THREADS) < T          # alone: the grid of its own pair
    ph = LC.stream_phases(R['one group']['n1'], LC.launch_threads(R['one group'], 'joint'))
    assert (ph['rem'], ph['threads']) == (1, L3_THREADS)
    ph = LC.stream_phases(R['whole grid']['n1'], LC.launch_threads(R['whole grid'], 'joint'))
    assert ph['rem'] == ph['threads'] == 2 * L3_THREADS and ph['rem_max'] == 1
    assert {r['tmode'] for r in LC.OBJECTIVE_ROWS} >= {'zeros', 'perfect'} and all(len(r['pairs']) >= 2 for r in LC.OBJECTIVE_ROWS)
    assert all(len(r['pairs']) == 4 for r in LC.OBJECTIVE_ROWS if max(r['n1'], r['n2']) < 100000)
    assert all(LC.NOT_IN_TABLE.values())
    # seg_counts_kernel<C, VEC>
    inst = {(r['C'], r['vec']) for r in LC.SEG_ROWS}
    assert inst == {(C, v) for C in (1, 2, 3, 4) for v in (False, True)}, inst
    for r in LC.SEG_ROWS:
        geo = LC.seg_geometry(r)
        assert geo['vec'] == r['vec'] and (r['blocks'] is None or r['blocks'] == (geo['want'], geo['launched'])), (r['id'], geo)
    S = LC.SEG_BY_ID
    assert all(LC.seg_geometry(S[k])['short'] for k in ('vec, short last group 2x4x5', 'vec, short last group 1x2x6', 'sample starts 3x2x6', 'sample starts 3x4x3'))
    assert not LC.seg_geometry(S['vec, whole groups 2x3x64'])['short'] and LC.seg_geometry(S['vec C1 2x1x1032'])['launched'] == 2
    by_base = S['scalar, by base 2x4x64']
    assert (by_base['P'] * by_base['C']) % 4 == 0 and by_base['offset'] % 4 != 0          # non-VEC by alignment alone
    cap = S['grid cap 64x3x33001']
    assert L3_MAX_BLOCKS // cap['B'] == cap['blocks'][1] < cap['blocks'][0]
    floor = [r for r in LC.SEG_ROWS if r['id'].startswith('cap floor')][0]
    assert floor['B'] > L3_MAX_BLOCKS and floor['blocks'] == (2, 1) and LC.seg_geometry(floor)['ngrp'] == 276
