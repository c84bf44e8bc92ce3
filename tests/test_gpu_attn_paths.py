"""Every form the dispatchers of csrc/mrdis_outdec.hip (channel attention with the skip sum, symmetric difference, residual gate) and of
csrc/mrdis_latent.hip (the masked KL term, the mean compaction) can reach, element by element against float64 (tests/attn_check.py), through the C ABI
(hip.load() and ctypes: the rows choose every leading dimension, pointer offset and workspace size themselves).

One row = one entry-point pair (forward and backward), one geometry, one layout.  A row is a function of an implementation object: HipImpl runs the
kernels, TorchImpl evaluates the same operation in plain fp32 torch on the CPU -- the yardstick.  tests/test_attn_check.py runs every row with
TorchImpl (no GPU) and holds attn_check.KAPPA to 4 x the worst yardstick ratio; the tests below run them with HipImpl under that table.

Every row with a pitch runs twice: dense, and through channel (KL: column) slices of wider buffers -- NaN beside every input slice, so that a read
of a neighbour poisons the result; outputs prefilled with NaN, whose neighbours must keep their NaN bits.  The slice of a row is 8 channels in on
both sides (the float4 forms stay float4) unless the row names its own (l, r): one channel in (scalar by alignment), ld = C + 2 (scalar by stride).
Every call asserts the launch counters: its own family once, 'elem_v1' exactly when chatt_vec chose the scalar forms, 'all' the launches the call
makes, every other counter 0.  Every chatt call runs twice (same bits) on a workspace over-allocated by 4 KB of NaN that must stay untouched.
Which pixel-chunk geometry a chatt call takes no counter sees: chatt_geom() below restates the source's rule and every row asserts the (CG, P,
last-group width) it claims against it.

MRDIS_DUMP_MEASURED=<dir> records both ratios of every row (attn_path_margins.jsonl; profiles/attn_path_margins.txt)."""
import ctypes as C_
import functools
import os
import re

import pytest
import torch
import torch.nn.functional as F

import attn_check as AT
from fixtures import dump_measured

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
NAN = float('nan')
MEASURING = bool(os.environ.get('MRDIS_DUMP_MEASURED'))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'representation-disentanglement_amd', 'csrc')
_OUTDEC = open(os.path.join(CSRC, 'mrdis_outdec.hip')).read()
OD_THREADS = int(re.search(r'constexpr int OD_THREADS = (\d+);', _OUTDEC).group(1))
RG_LANES = int(re.search(r'constexpr int RG_LANES = (\d+);', _OUTDEC).group(1))
KL_MAXM = int(re.search(r'#define MRDIS_KL_MAXM (\d+)', open(os.path.join(ROOT, 'include', 'mrdis.h')).read()).group(1))
GRID_CAP = 8192          # od_grid / lat_grid
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
DENSE, SLICE = (0, 0), (8, 8)
G_UP = 2.5               # the upstream gradient of the KL rows (a device scalar)

# what the table leaves out, and why
NOT_IN_TABLE = {
    'kl_bwd: the grid-stride of the prior-gradient blocks': 'one thread per (i, z) of a broadcast prior; the blocks stride only beyond M Z > 8192 x 256 '
                                                            '(2M), with M <= 8 a Z of 262145: no latent code is near that and the row would move 17 GB',
}


@pytest.fixture(autouse=True)
def _cpu_threads():
    """the float64 references on at most 16 CPU threads"""
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    yield
    torch.set_num_threads(n)


def rnd(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def bits_eq(a, b, what):
    AT.assert_same_bits(a.detach().cpu().contiguous(), b.detach().cpu().contiguous(), what)


def is_zero(t, what):
    assert not bool(t.any()), f'{what}: {int((t != 0).sum())} of {t.numel()} elements are not exactly 0'


def is_nan_bits(t, what):
    nan = torch.full((1,), NAN).view(torch.int32).item()
    assert bool((t.contiguous().view(torch.int32) == nan).all()), f'{what}: a store landed outside the output'


class Rec:
    """collects (output, kappa key, ratio) of one row; enforce: every output is held to its committed kappa"""

    def __init__(self, rid, enforce):
        self.rid, self.enforce, self.items = rid, enforce, []

    def __call__(self, name, key, got, ref, A):
        if self.enforce:
            assert key in AT.KAPPA, f'no kappa committed for {key}'
            r = AT.check(got, ref, A, AT.KAPPA[key], what=f'{self.rid}: {name}')
        else:
            r = AT.ratio(got, ref, A)
        self.items.append((name, key, r))


def is_v1(C, lay):
    """chatt_vec: the scalar forms for C % 4, a view not 16-byte aligned (the buffers themselves are) or a stride % 4"""
    l, r = lay
    return bool(C % 4 or l % 4 or (l + C + r) % 4)


def chatt_geom(B, HW, C, V):
    """the source's chatt_geom, plus the width of the last channel group"""
    CV = C // V
    CG = -(-CV // OD_THREADS)
    P = max(1, min(1024 // (B * CG), max(HW // 64, 1)))
    chunk = -(-HW // P)
    return dict(CG=CG, P=-(-HW // chunk), chunk=chunk, last=CV - (CG - 1) * OD_THREADS)


# ================================================================ implementations
class TorchImpl:
    """plain fp32 torch on the CPU: the yardstick.  Layouts do not apply (there is one dense evaluation)"""
    gpu = False

    def chatt_fwd(self, c, lay):
        return AT.chatt_fwd_t(c['x'], c['s'], c['wd'], c['bd'], c['wu'], c['bu'])

    def chatt_bwd(self, c, f, lay):
        return AT.chatt_bwd_t(c['dy'], c['x'], f['a'], f['hid'], f['pool'], c['wd'], c['wu'])

    def symdiff_fwd(self, g, lay):
        return (g - g.flip(1)).abs()

    def symdiff_bwd(self, dgd, g, lay):
        gr = g.clone().requires_grad_(True)
        return torch.autograd.grad(((gr - gr.flip(1)).abs() * dgd).sum(), gr)[0]

    def rgate_fwd(self, x, alpha, lay):
        return (1 + AT.up2(alpha)) * x

    def rgate_bwd(self, dy, x, alpha, lay):
        o = AT.rgate_bwd_t(dy, x, alpha)
        return o['dx'], o['rsum']

    def rgate_dalpha(self, dy, x, alpha):
        return AT.rgate_bwd_t(dy, x, alpha)['dalpha']

    def kl(self, c, lay):
        o = AT.kl_t(c['mu'], c['lv'], c['w'], c['pm'], c['plv'], G_UP)
        if not c['need_prior']:
            o.pop('dpmu', None); o.pop('dplv', None)
        return o

    def avgpool_fwd(self, x, k, lay):
        return F.avg_pool2d(x.permute(0, 3, 1, 2), k).reshape(x.shape[0], -1)

    def avgpool_bwd(self, dy, shape, k, lay):
        N, H, W, C = shape
        xr = torch.zeros(N, C, H, W, requires_grad=True)
        return torch.autograd.grad((F.avg_pool2d(xr, k).reshape(N, -1) * dy).sum(), xr)[0].permute(0, 2, 3, 1).contiguous()

    def refusals(self):
        return None


def d_(t):
    return t.to(DEV).contiguous()


def ptr_array(ts, off_bytes=0):
    return (C_.c_void_p * len(ts))(*[None if t is None else t.data_ptr() + off_bytes for t in ts])


class HipImpl:
    """the kernels under test, through the C ABI.  lay = (l, r): an operand of C channels is columns [l, l + C) of an (P, l + C + r) buffer"""
    gpu = True

    def __init__(self, m):
        self.hip, self.lib = m.hip, m.hip.load()

    def st(self):
        return self.hip._stream()

    def put(self, t, lay):
        """-> (view (P, C), ld): the input as a column slice, NaN beside it"""
        l, r = lay
        t = t.reshape(-1, t.shape[-1])
        P, C = t.shape
        buf = torch.full((P, l + C + r), NAN, device=DEV)
        buf[:, l:l + C] = t.to(DEV)
        return buf[:, l:l + C], l + C + r

    def out(self, P, C, lay):
        l, r = lay
        buf = torch.full((P, l + C + r), NAN, device=DEV)
        return buf, buf[:, l:l + C], l + C + r

    def done(self, buf, view, lay, what):
        l, r = lay
        C = view.shape[1]
        if l:
            is_nan_bits(buf[:, :l], what)
        if r:
            is_nan_bits(buf[:, l + C:], what)
        return view.cpu().contiguous()

    def call(self, fam, v1, launches, fn, *args):
        """one accepted call and its counters: the family once, elem_v1 for the scalar forms, 'all' the launches, nothing else"""
        self.hip.launch_counts(reset=True)
        rc = fn(*args)
        assert rc == 0, (fn.__name__, rc)
        got = {k: n for k, n in self.hip.launch_counts(reset=True, elem=True).items() if n}
        want = {fam: 1, 'all': launches}
        if v1:
            want['elem_v1'] = 1
        assert got == want, f'{fn.__name__}: counted {got}, the row expects {want}'

    # ---- channel attention
    def chatt_ws(self, B, HW, C, Hd):
        nb = self.lib.mrdis_chatt_workspace(B, HW, C, Hd)
        assert nb > 0 and nb % 4 == 0
        return torch.full((nb // 4 + 1024,), NAN, device=DEV), nb

    def chatt_fwd(self, c, lay):
        lib = self.lib
        B, HW, C = c['x'].shape
        Hd = c['wd'].shape[0]
        (xv, ldx), (sv, lds) = self.put(c['x'], lay), self.put(c['s'], lay)
        wd, bd, wu, bu = (d_(c[k]) for k in ('wd', 'bd', 'wu', 'bu'))
        runs = []
        for _ in range(2):
            obuf, o, ldo = self.out(B * HW, C, lay)
            pool, hid, a = (torch.full(s, NAN, device=DEV) for s in ((B, C), (B, Hd), (B, C)))
            ws, nb = self.chatt_ws(B, HW, C, Hd)
            self.call('chatt', is_v1(C, lay), 3, lib.mrdis_chatt_fwd, xv.data_ptr(), ldx, sv.data_ptr(), lds, wd.data_ptr(), bd.data_ptr(), wu.data_ptr(), bu.data_ptr(),
                      o.data_ptr(), ldo, pool.data_ptr(), hid.data_ptr(), a.data_ptr(), ws.data_ptr(), nb, B, HW, C, Hd, self.st())
            is_nan_bits(ws[nb // 4:], 'chatt_fwd workspace tail')
            runs.append(dict(out=self.done(obuf, o, lay, 'chatt out').reshape(B, HW, C), pool=pool.cpu(), hid=hid.cpu(), a=a.cpu()))
        for k in runs[0]:
            bits_eq(runs[1][k], runs[0][k], f'chatt_fwd {k}: second call')
        return runs[0]

    def chatt_bwd(self, c, f, lay):
        lib = self.lib
        B, HW, C = c['x'].shape
        Hd = c['wd'].shape[0]
        (dyv, lddy), (xv, ldx) = self.put(c['dy'], lay), self.put(c['x'], lay)
        a, hid, pool, wd, wu = (d_(t) for t in (f['a'], f['hid'], f['pool'], c['wd'], c['wu']))
        runs = []
        for _ in range(2):
            xbuf, dx, lddx = self.out(B * HW, C, lay)
            dwd, dbd, dwu, dbu = (torch.full(s, NAN, device=DEV) for s in ((Hd, C), (Hd,), (C, Hd), (C,)))
            ws, nb = self.chatt_ws(B, HW, C, Hd)
            self.call('chatt', is_v1(C, lay), 3, lib.mrdis_chatt_bwd, dyv.data_ptr(), lddy, xv.data_ptr(), ldx, a.data_ptr(), hid.data_ptr(), pool.data_ptr(), wd.data_ptr(),
                      wu.data_ptr(), dx.data_ptr(), lddx, dwd.data_ptr(), dbd.data_ptr(), dwu.data_ptr(), dbu.data_ptr(), ws.data_ptr(), nb, B, HW, C, Hd, self.st())
            is_nan_bits(ws[nb // 4:], 'chatt_bwd workspace tail')
            runs.append(dict(dx=self.done(xbuf, dx, lay, 'chatt dx').reshape(B, HW, C), dwd=dwd.cpu(), dbd=dbd.cpu(), dwu=dwu.cpu(), dbu=dbu.cpu()))
        for k in runs[0]:
            bits_eq(runs[1][k], runs[0][k], f'chatt_bwd {k}: second call')
        return runs[0]

    # ---- symmetric difference
    def symdiff_fwd(self, g, lay):
        B, H, W, C = g.shape
        gv, ldg = self.put(g, lay)
        buf, o, ldo = self.out(B * H * W, C, lay)
        self.call('symdiff', is_v1(C, lay), 1, self.lib.mrdis_symdiff_fwd, gv.data_ptr(), ldg, o.data_ptr(), ldo, B, H, W, C, self.st())
        return self.done(buf, o, lay, 'symdiff gd').reshape(B, H, W, C)

    def symdiff_bwd(self, dgd, g, lay):
        B, H, W, C = g.shape
        (dv, ldd), (gv, ldg) = self.put(dgd, lay), self.put(g, lay)
        buf, o, ldo = self.out(B * H * W, C, lay)
        self.call('symdiff', is_v1(C, lay), 1, self.lib.mrdis_symdiff_bwd, dv.data_ptr(), ldd, gv.data_ptr(), ldg, o.data_ptr(), ldo, B, H, W, C, self.st())
        return self.done(buf, o, lay, 'symdiff dg').reshape(B, H, W, C)

    # ---- residual gate
    def rgate_fwd(self, x, alpha, lay):
        B, H, W, C = x.shape
        xv, ldx = self.put(x, lay)
        buf, o, ldo = self.out(B * H * W, C, lay)
        self.call('rgate', is_v1(C, lay), 1, self.lib.mrdis_rgate_fwd, xv.data_ptr(), ldx, d_(alpha).data_ptr(), o.data_ptr(), ldo, B, H, W, C, self.st())
        return self.done(buf, o, lay, 'rgate out').reshape(B, H, W, C)

    def rgate_bwd(self, dy, x, alpha, lay):
        B, H, W, C = x.shape
        (dv, ldd), (xv, ldx) = self.put(dy, lay), self.put(x, lay)
        buf, dx, lddx = self.out(B * H * W, C, lay)
        rsum = torch.full((B, H, W), NAN, device=DEV)
        self.call('rgate', is_v1(C, lay), 1, self.lib.mrdis_rgate_bwd, dv.data_ptr(), ldd, xv.data_ptr(), ldx, d_(alpha).data_ptr(), dx.data_ptr(), lddx, rsum.data_ptr(),
                  B, H, W, C, self.st())
        return self.done(buf, dx, lay, 'rgate dx').reshape(B, H, W, C), rsum.cpu()

    def rgate_dalpha(self, dy, x, alpha):
        """the wrapper: rsum, then the bilinear backward"""
        nchw = lambda t: t.to(DEV).permute(0, 3, 1, 2)          # (channels_last views)
        _, dal = self.hip.rgate_bwd(nchw(dy), nchw(x), alpha.to(DEV)[:, None])
        return dal[:, 0].cpu()

    # ---- KL
    def kl(self, c, lay):
        lib = self.lib
        mu, lv = c['mu'], c['lv']
        M, B, Z = mu.shape
        IN = 3          # mu / lv: row stride Z + 3, NaN behind every row

        def wide(t, pad):
            buf = torch.full(tuple(t.shape[:-1]) + (Z + pad,), NAN, device=DEV)
            buf[..., :Z] = t.to(DEV)
            return buf
        wmu, wlv, w = wide(mu, IN), wide(lv, IN), d_(c['w'])
        mus, lvs = ptr_array(list(wmu)), ptr_array(list(wlv))
        pmu = plv = None
        ldp_m = ldp_b = 0
        if c['pm'] is not None:
            pmu, plv = wide(c['pm'], c['pp']), wide(c['plv'], c['pp'])
            if c['pm'].dim() == 3:
                ldp_b, ldp_m = Z + c['pp'], B * (Z + c['pp'])
            else:
                ldp_m = Z + c['pp']
        pp = lambda t: None if t is None else t.data_ptr()
        losses = []
        for _ in range(2):
            loss = torch.full((1,), NAN, device=DEV)
            self.call('kl', False, 1, lib.mrdis_kl_fwd, mus, lvs, Z + IN, Z + IN, pp(pmu), pp(plv), ldp_m, ldp_b, w.data_ptr(), loss.data_ptr(), M, B, Z, self.st())
            losses.append(loss.cpu())
        bits_eq(losses[1], losses[0], 'kl loss: second call')
        l, r = lay
        dmu, dlv = (torch.full((M, B, l + Z + r), NAN, device=DEV) for _ in range(2))
        dpmu = dplv = None
        if c['pm'] is not None and c['need_prior']:
            dpmu, dplv = (torch.full(tuple(c['pm'].shape), NAN, device=DEV) for _ in range(2))
        g = torch.full((1,), G_UP, device=DEV)
        self.call('kl', False, 1, lib.mrdis_kl_bwd, g.data_ptr(), mus, lvs, Z + IN, Z + IN, pp(pmu), pp(plv), ldp_m, ldp_b, w.data_ptr(),
                  ptr_array(list(dmu), 4 * l), ptr_array(list(dlv), 4 * l), l + Z + r, l + Z + r, pp(dpmu), pp(dplv), M, B, Z, self.st())
        o = dict(loss=losses[0])
        for name, buf in (('dmu', dmu), ('dlv', dlv)):
            o[name] = self.done(buf.reshape(M * B, -1), buf.reshape(M * B, -1)[:, l:l + Z], lay, 'kl ' + name).reshape(M, B, Z)
        if dpmu is not None:
            o.update(dpmu=dpmu.cpu(), dplv=dplv.cpu())
        return o

    # ---- mean compaction
    def avgpool_fwd(self, x, k, lay):
        N, H, W, C = x.shape
        xv, ldx = self.put(x, lay)
        y = torch.full((N, C * (H // k) * (W // k)), NAN, device=DEV)
        self.call('avgpool', False, 1, self.lib.mrdis_avgpool_fwd, xv.data_ptr(), ldx, y.data_ptr(), N, H, W, C, k, self.st())
        return y.cpu()

    def avgpool_bwd(self, dy, shape, k, lay):
        N, H, W, C = shape
        buf, dx, lddx = self.out(N * H * W, C, lay)
        self.call('avgpool', False, 1, self.lib.mrdis_avgpool_bwd, d_(dy).data_ptr(), dx.data_ptr(), lddx, N, H, W, C, k, self.st())
        return self.done(buf, dx, lay, 'avgpool dx').reshape(N, H, W, C)

    # ---- refusals: host-side argument checks that launch nothing
    def refusals(self):
        """-> [(what, return code, the code the source gives, counters that moved)] of every refused call and of one accepted control call per
        entry point (the same arguments without the one override; into a second buffer), then the refused calls' output buffer must still be NaN"""
        lib, hip, st = self.lib, self.hip, self.st()
        zin = torch.zeros(1 << 16, device=DEV)                          # every input pointer: zeros
        nout, ctl = (torch.full((1 << 16,), NAN, device=DEV) for _ in range(2))
        SLOT = 4096 * 4                                                 # outputs sit 4096 floats apart
        res = []

        def run(what, want, fn, args, counted=()):
            hip.launch_counts(reset=True)
            rc = fn(*args)
            moved = {k: n for k, n in hip.launch_counts(reset=True, elem=True).items() if n and k not in counted}
            res.append((what, rc, want, moved))

        def table(name, fn, order, base, outs, cases, fam, launches):
            """base: name -> value; outs: the output pointers' names; cases: [(what, code, overrides)]"""
            def args(buf, over):
                a = dict(base)
                a.update({n: buf.data_ptr() + i * SLOT for i, n in enumerate(outs)})
                a.update(over)
                for k, v in list(a.items()):
                    if callable(v):
                        a[k] = v(a)
                return [a[k] for k in order] + [st]
            for what, code, over in cases:
                run(f'{name}: {what}', code, fn, args(nout, over))
            run(f'{name}: control', 0, fn, args(ctl, {}), counted=(fam, 'all'))
            assert hip.launch_counts()[fam] == 0

        z = zin.data_ptr()
        need = lambda a: lib.mrdis_chatt_workspace(a['B'], a['HW'], a['C'], a['Hd'])
        # chatt
        cb = dict(x=z, ldx=8, s=z, lds=8, wd=z, bd=z, wu=z, bu=z, ldo=8, nb=need, B=2, HW=6, C=8, Hd=2)
        wide = dict(C=4097, ldx=4097, lds=4097, ldo=4097, B=1, HW=1)
        table('chatt_fwd', lib.mrdis_chatt_fwd, ['x', 'ldx', 's', 'lds', 'wd', 'bd', 'wu', 'bu', 'out', 'ldo', 'pool', 'hid', 'a', 'ws', 'nb', 'B', 'HW', 'C', 'Hd'], cb,
              ['out', 'pool', 'hid', 'a', 'ws'],
              [('ldx < C', EINVAL, dict(ldx=7)), ('lds < C', EINVAL, dict(lds=7)), ('ldo < C', EINVAL, dict(ldo=7)), ('x NULL', EINVAL, dict(x=None)), ('s NULL', EINVAL, dict(s=None)),
               ('W_down NULL', EINVAL, dict(wd=None)), ('b_up NULL', EINVAL, dict(bu=None)), ('out NULL', EINVAL, dict(out=None)), ('pool NULL', EINVAL, dict(pool=None)),
               ('a NULL', EINVAL, dict(a=None)), ('workspace NULL', EINVAL, dict(ws=None)), ('B = 0', EINVAL, dict(B=0, nb=1 << 16)), ('C = 4097', EUNSUPPORTED, wide),
               ('Hd = 1025', EUNSUPPORTED, dict(Hd=1025)), ('ws_bytes one short', EWORKSPACE, dict(nb=lambda a: need(a) - 1))], 'chatt', 3)
        cb = dict(dy=z, lddy=8, x=z, ldx=8, a=z, hid=z, pool=z, wd=z, wu=z, lddx=8, nb=need, B=2, HW=6, C=8, Hd=2)
        wide = dict(C=4097, lddy=4097, ldx=4097, lddx=4097, B=1, HW=1)
        table('chatt_bwd', lib.mrdis_chatt_bwd, ['dy', 'lddy', 'x', 'ldx', 'a', 'hid', 'pool', 'wd', 'wu', 'dx', 'lddx', 'dwd', 'dbd', 'dwu', 'dbu', 'ws', 'nb', 'B', 'HW', 'C', 'Hd'],
              cb, ['dx', 'dwd', 'dbd', 'dwu', 'dbu', 'ws'],
              [('lddy < C', EINVAL, dict(lddy=7)), ('ldx < C', EINVAL, dict(ldx=7)), ('lddx < C', EINVAL, dict(lddx=7)), ('dy NULL', EINVAL, dict(dy=None)), ('x NULL', EINVAL, dict(x=None)),
               ('a NULL', EINVAL, dict(a=None)), ('hid NULL', EINVAL, dict(hid=None)), ('W_up NULL', EINVAL, dict(wu=None)), ('dx NULL', EINVAL, dict(dx=None)),
               ('dW_down NULL', EINVAL, dict(dwd=None)), ('db_up NULL', EINVAL, dict(dbu=None)), ('workspace NULL', EINVAL, dict(ws=None)), ('C = 4097', EUNSUPPORTED, wide),
               ('Hd = 1025', EUNSUPPORTED, dict(Hd=1025)), ('ws_bytes one short', EWORKSPACE, dict(nb=lambda a: need(a) - 1))], 'chatt', 3)
        # symdiff
        sb = dict(g=z, ldg=8, ldo=8, B=2, H=3, W=2, C=8)
        table('symdiff_fwd', lib.mrdis_symdiff_fwd, ['g', 'ldg', 'gd', 'ldo', 'B', 'H', 'W', 'C'], sb, ['gd'],
              [('ldg < C', EINVAL, dict(ldg=7)), ('ldo < C', EINVAL, dict(ldo=7)), ('g NULL', EINVAL, dict(g=None)), ('gd NULL', EINVAL, dict(gd=None)), ('H = 0', EINVAL, dict(H=0))],
              'symdiff', 1)
        sb = dict(dgd=z, lddgd=8, g=z, ldg=8, lddg=8, B=2, H=3, W=2, C=8)
        table('symdiff_bwd', lib.mrdis_symdiff_bwd, ['dgd', 'lddgd', 'g', 'ldg', 'dg', 'lddg', 'B', 'H', 'W', 'C'], sb, ['dg'],
              [('lddgd < C', EINVAL, dict(lddgd=7)), ('ldg < C', EINVAL, dict(ldg=7)), ('lddg < C', EINVAL, dict(lddg=7)), ('dgd NULL', EINVAL, dict(dgd=None)),
               ('g NULL', EINVAL, dict(g=None)), ('dg NULL', EINVAL, dict(dg=None))], 'symdiff', 1)
        # rgate
        rb = dict(x=z, ldx=8, alpha=z, ldo=8, B=2, H=4, W=2, C=8)
        table('rgate_fwd', lib.mrdis_rgate_fwd, ['x', 'ldx', 'alpha', 'out', 'ldo', 'B', 'H', 'W', 'C'], rb, ['out'],
              [('odd H', EINVAL, dict(H=3)), ('odd W', EINVAL, dict(W=3)), ('H = 0', EINVAL, dict(H=0)), ('ldx < C', EINVAL, dict(ldx=7)), ('ldo < C', EINVAL, dict(ldo=7)),
               ('x NULL', EINVAL, dict(x=None)), ('alpha NULL', EINVAL, dict(alpha=None)), ('out NULL', EINVAL, dict(out=None))], 'rgate', 1)
        rb = dict(dy=z, lddy=8, x=z, ldx=8, alpha=z, lddx=8, B=2, H=4, W=2, C=8)
        table('rgate_bwd', lib.mrdis_rgate_bwd, ['dy', 'lddy', 'x', 'ldx', 'alpha', 'dx', 'lddx', 'rsum', 'B', 'H', 'W', 'C'], rb, ['dx', 'rsum'],
              [('odd H', EINVAL, dict(H=3)), ('odd W', EINVAL, dict(W=3)), ('H = 0', EINVAL, dict(H=0)), ('lddy < C', EINVAL, dict(lddy=7)), ('ldx < C', EINVAL, dict(ldx=7)),
               ('lddx < C', EINVAL, dict(lddx=7)), ('dy NULL', EINVAL, dict(dy=None)), ('alpha NULL', EINVAL, dict(alpha=None)), ('dx NULL', EINVAL, dict(dx=None)),
               ('rsum NULL', EINVAL, dict(rsum=None))], 'rgate', 1)
        # KL: M = 2 blocks of (B, Z) = (3, 4) inside the zero buffer; the gradient blocks 64 floats apart inside their output slot
        M, B, Z = 2, 3, 4
        ins = lambda n=M, hole=None: (C_.c_void_p * n)(*[None if i == hole else z + 256 * i for i in range(n)])
        outs_ = lambda name: (lambda a: (C_.c_void_p * M)(*[a[name + '_slot'] + 256 * i for i in range(M)]))
        kb = dict(mu=ins(), lv=ins(), ldmu=Z, ldlv=Z, pmu=z, plv=z, ldp_m=Z, ldp_b=0, w=z, M=M, B=B, Z=Z)
        kl_cases = [('M = 9', EUNSUPPORTED, dict(M=KL_MAXM + 1, mu=ins(KL_MAXM + 1), lv=ins(KL_MAXM + 1))), ('ldmu < Z', EINVAL, dict(ldmu=Z - 1)), ('ldlv < Z', EINVAL, dict(ldlv=Z - 1)),
                    ('0 < ldp_b < Z', EINVAL, dict(ldp_b=Z - 1)), ('pmu without plv', EINVAL, dict(plv=None)), ('plv without pmu', EINVAL, dict(pmu=None)),
                    ('mu array NULL', EINVAL, dict(mu=None)), ('a NULL block in lv', EINVAL, dict(lv=ins(hole=1))), ('weight NULL', EINVAL, dict(w=None)), ('Z = 0', EINVAL, dict(Z=0))]
        table('kl_fwd', lib.mrdis_kl_fwd, ['mu', 'lv', 'ldmu', 'ldlv', 'pmu', 'plv', 'ldp_m', 'ldp_b', 'w', 'loss', 'M', 'B', 'Z'], kb, ['loss'],
              kl_cases + [('loss NULL', EINVAL, dict(loss=None))], 'kl', 1)
        kb = dict(kb, dloss=z, dmu=outs_('dmu'), dlv=outs_('dlv'), lddmu=Z, lddlv=Z)
        table('kl_bwd', lib.mrdis_kl_bwd, ['dloss', 'mu', 'lv', 'ldmu', 'ldlv', 'pmu', 'plv', 'ldp_m', 'ldp_b', 'w', 'dmu', 'dlv', 'lddmu', 'lddlv', 'dpmu', 'dplv', 'M', 'B', 'Z'],
              kb, ['dmu_slot', 'dlv_slot', 'dpmu', 'dplv'],
              kl_cases + [('lddmu < Z', EINVAL, dict(lddmu=Z - 1)), ('lddlv < Z', EINVAL, dict(lddlv=Z - 1)), ('dloss NULL', EINVAL, dict(dloss=None)),
                          ('dmu array NULL', EINVAL, dict(dmu=None)), ('dpmu without a prior', EINVAL, dict(pmu=None, plv=None)), ('dpmu without dplv', EINVAL, dict(dplv=None)),
                          ('dplv without dpmu', EINVAL, dict(dpmu=None))], 'kl', 1)
        # avgpool
        ab = dict(x=z, ldx=8, N=2, H=4, W=6, C=8, k=2)
        table('avgpool_fwd', lib.mrdis_avgpool_fwd, ['x', 'ldx', 'y', 'N', 'H', 'W', 'C', 'k'], ab, ['y'],
              [('k > H', EINVAL, dict(k=5)), ('k = 0', EINVAL, dict(k=0)), ('ldx < C', EINVAL, dict(ldx=7)), ('x NULL', EINVAL, dict(x=None)), ('y NULL', EINVAL, dict(y=None))], 'avgpool', 1)
        ab = dict(dy=z, lddx=8, N=2, H=4, W=6, C=8, k=2)
        table('avgpool_bwd', lib.mrdis_avgpool_bwd, ['dy', 'dx', 'lddx', 'N', 'H', 'W', 'C', 'k'], ab, ['dx'],
              [('k > H', EINVAL, dict(k=5)), ('k > W', EINVAL, dict(k=3, H=3, W=2)), ('k = 0', EINVAL, dict(k=0)), ('lddx < C', EINVAL, dict(lddx=7)), ('dy NULL', EINVAL, dict(dy=None)),
               ('dx NULL', EINVAL, dict(dx=None))], 'avgpool', 1)
        torch.cuda.synchronize()
        is_nan_bits(nout, 'a refused call wrote')
        assert not bool(torch.isnan(ctl).all()), 'the control calls wrote nothing'
        return res


# ================================================================ rows
def lay_tag(lay):
    return 'dense' if lay == DENSE else 'slice'


# ---------------------------------------------------------------- channel attention
def CH(rid, B, C, H, W, Hd, V, CG, P, last, lay=SLICE, dense=None):
    """V, CG, P, last: the form and pixel-chunk geometry of the SLICE run; dense: the same of the dense run where it differs"""
    return pytest.param(dict(B=B, C=C, H=H, W=W, Hd=Hd, lay=lay, geom=dict(V=V, CG=CG, P=P, last=last), dense=dense or dict(V=V, CG=CG, P=P, last=last)), id=rid)


CHATT_ROWS = [
    CH('chatt 2x64x5x6 Hd16 float4 P1', 2, 64, 5, 6, 16, 4, 1, 1, 16),
    CH('chatt 2x64x10x20 Hd16 three chunks 67 67 66', 2, 64, 10, 20, 16, 4, 1, 3, 16),
    CH('chatt 1x1028x8x9 Hd8 float4 CG2 last group one vector', 1, 1028, 8, 9, 8, 4, 2, 1, 1),
    CH('chatt 2x40x7x9 Hd5 CV10 idle lanes', 2, 40, 7, 9, 5, 4, 1, 1, 10),
    CH('chatt 2x6x5x6 Hd3 scalar by C', 2, 6, 5, 6, 3, 1, 1, 1, 6),
    CH('chatt 2x64x8x8 Hd16 offset 1 scalar by alignment', 2, 64, 8, 8, 16, 1, 1, 1, 64, lay=(1, 3), dense=dict(V=4, CG=1, P=1, last=16)),
    CH('chatt 2x64x8x8 Hd16 ld C+2 scalar by stride', 2, 64, 8, 8, 16, 1, 1, 1, 64, lay=(0, 2), dense=dict(V=4, CG=1, P=1, last=16)),
    CH('chatt 1x260x9x8 Hd4 offset 1 scalar CG2 last group 4', 1, 260, 9, 8, 4, 1, 2, 1, 4, lay=(1, 3), dense=dict(V=4, CG=1, P=1, last=65)),
    CH('chatt 2x12x6x5 Hd1 scalar CVb12', 2, 12, 6, 5, 1, 1, 1, 1, 12, lay=(1, 3), dense=dict(V=4, CG=1, P=1, last=3)),
    CH('chatt 1025x4x2x2 Hd2 B CG over 1024', 1025, 4, 2, 2, 2, 4, 1, 1, 1),
    CH('chatt 64x64x32x33 Hd16 P16 grid-stride', 64, 64, 32, 33, 16, 4, 1, 16, 16),
    CH('chatt 3x8x1x1 Hd2 HW1', 3, 8, 1, 1, 2, 4, 1, 1, 2),
]


@functools.lru_cache(maxsize=2)
def chatt_case(B, C, HW, Hd):
    g = torch.Generator().manual_seed(1000 + C + HW)
    r = lambda *s: torch.randn(*s, generator=g)
    c = dict(x=r(B, HW, C), s=r(B, HW, C), dy=r(B, HW, C), wd=r(Hd, C) / C ** 0.5, bd=0.1 * r(Hd), wu=r(C, Hd) / Hd ** 0.5, bu=0.1 * r(C))
    if C > 1:          # one channel a million times smaller than its neighbours: a max-scaled bound does not see it
        for k in ('x', 's', 'dy'):
            c[k][:, :, 1] *= 1e-6
    return c


def row_chatt(row, impl, rec):
    B, C, H, W, Hd = (row[k] for k in ('B', 'C', 'H', 'W', 'Hd'))
    HW = H * W
    c = chatt_case(B, C, HW, Hd)
    pool_ref = AT.chatt_pool_ref(c['x'])
    for lay, geom in ((DENSE, row['dense']), (row['lay'], row['geom'])):
        tag = ' ' + lay_tag(lay)
        assert geom['V'] == (1 if is_v1(C, lay) else 4), 'the row states the wrong form'
        g = chatt_geom(B, HW, C, geom['V'])
        assert {k: geom[k] for k in ('CG', 'P', 'last')} == {k: g[k] for k in ('CG', 'P', 'last')}, ('the row states the wrong geometry', geom, g)
        f = impl.chatt_fwd(c, lay)
        rec('pool' + tag, ('chatt', 'pool'), f['pool'], *pool_ref)
        rec('hid' + tag, ('chatt', 'hid'), f['hid'], *AT.chatt_hid_ref(f['pool'], c['wd'], c['bd']))          # each stage from the STORED stage in front
        rec('a' + tag, ('chatt', 'a'), f['a'], *AT.chatt_a_ref(f['hid'], c['wu'], c['bu']))
        rec('out' + tag, ('chatt', 'out'), f['out'], *AT.chatt_out_ref(c['x'], c['s'], f['a']))
        b = impl.chatt_bwd(c, f, lay)
        ref = AT.chatt_bwd_ref(c['dy'], c['x'], f['a'], f['hid'], f['pool'], c['wd'], c['wu'])
        for n in ('dx', 'dwd', 'dbd', 'dwu', 'dbu'):
            rec(n + tag, ('chatt', n), b[n], *ref[n])


# ---------------------------------------------------------------- symmetric difference
def SD(rid, B, C, H, W, v1=False, big=False):
    """v1: the scalar forms (elem_v1 counts 1 per call), dense and slice alike"""
    return pytest.param(dict(B=B, C=C, H=H, W=W, v1=v1, big=big), id=rid)


SYMDIFF_ROWS = [
    SD('symdiff 2x64x5x6 odd H', 2, 64, 5, 6), SD('symdiff 2x64x8x8', 2, 64, 8, 8), SD('symdiff 2x6x5x6 scalar', 2, 6, 5, 6, v1=True), SD('symdiff 1x8x1x7 H1', 1, 8, 1, 7),
    SD('symdiff 2x64x257x256 float4 over the grid cap', 2, 64, 257, 256, big=True), SD('symdiff 3x6x343x340 scalar over the grid cap', 3, 6, 343, 340, v1=True, big=True),
]


def row_symdiff(row, impl, rec):
    B, C, H, W = (row[k] for k in ('B', 'C', 'H', 'W'))
    assert row['big'] == (B * H * W * (C // (1 if C % 4 else 4)) > GRID_CAP * OD_THREADS), 'the row states the wrong side of the grid cap'
    g, dgd = rnd((B, H, W, C), 11), rnd((B, H, W, C), 12)
    g[:, 0, :, 0] = g[:, H - 1, :, 0]          # equal mirror rows in channel 0: sgn(0) = 0 away from the middle row too
    want = AT.symdiff_fwd_bits(g)
    ref = AT.symdiff_bwd_ref(dgd, g)
    for lay in (DENSE, SLICE):
        tag = ' ' + lay_tag(lay)
        assert row['v1'] == is_v1(C, lay), 'the row states the wrong form'
        bits_eq(impl.symdiff_fwd(g, lay), want, 'symdiff forward' + tag)
        dg = impl.symdiff_bwd(dgd, g, lay)
        rec('dg' + tag, ('symdiff', 'dg'), dg, *ref)
        is_zero(dg[:, 0, :, 0], 'dg where the mirror rows are equal'); is_zero(dg[:, H - 1, :, 0], 'dg where the mirror rows are equal')
        if H % 2:
            is_zero(dg[:, H // 2], 'dg on the middle row')          # (all of H = 1)


# ---------------------------------------------------------------- residual gate
def RG(rid, B, C, h, w, lay=SLICE, v1=(False, False), big=(False, False), dalpha=False):
    """v1: the scalar forms (elem_v1 counts 1 per call) of the (dense, slice) run; big: (forward, backward) beyond the grid cap"""
    return pytest.param(dict(B=B, C=C, h=h, w=w, lay=lay, v1=v1, big=big, dalpha=dalpha), id=rid)


RGATE_ROWS = [
    RG('rgate 2x64 gate 5x6', 2, 64, 5, 6, dalpha=True), RG('rgate 2x4 gate 1x1', 2, 4, 1, 1), RG('rgate 2x40 gate 1x7 CV10', 2, 40, 1, 7),
    RG('rgate 1x68 gate 3x1 CV17 lane 0 takes two', 1, 68, 3, 1), RG('rgate 2x6 gate 5x6 scalar', 2, 6, 5, 6, v1=(True, True)), RG('rgate 2x64 gate 4x4 ld C+2 scalar by stride', 2, 64, 4, 4, lay=(0, 2), v1=(False, True)),
    RG('rgate 2x4 gate 129x128 backward over the grid cap', 2, 4, 129, 128, big=(False, True)), RG('rgate 2x64 gate 129x128 forward over the grid cap', 2, 64, 129, 128, big=(True, True)),
]


def row_rgate(row, impl, rec):
    B, C, h, w = (row[k] for k in ('B', 'C', 'h', 'w'))
    H, W = 2 * h, 2 * w
    V = 1 if C % 4 else 4
    assert row['big'] == (B * H * W * (C // V) > GRID_CAP * OD_THREADS, B * H * W > GRID_CAP * (OD_THREADS // RG_LANES)), 'the row states the wrong side of the grid caps'
    x, dy, alpha = rnd((B, H, W, C), 21), rnd((B, H, W, C), 22), rnd((B, h, w), 23, 0.7)
    fref, bref = AT.rgate_fwd_ref(x, alpha), AT.rgate_bwd_ref(dy, x, alpha)
    for lay, v1 in zip((DENSE, row['lay']), row['v1']):
        tag = ' ' + lay_tag(lay)
        assert v1 == is_v1(C, lay), 'the row states the wrong form'
        rec('out' + tag, ('rgate', 'out'), impl.rgate_fwd(x, alpha, lay), *fref)
        dx, rsum = impl.rgate_bwd(dy, x, alpha, lay)
        rec('dx' + tag, ('rgate', 'dx'), dx, *bref['dx'])
        rec('rsum' + tag, ('rgate', 'rsum'), rsum, *bref['rsum'])
    if row['dalpha']:          # once, through the wrapper: rsum into the bilinear backward that tests/test_gpu_elem_paths.py covers
        rec('dalpha', ('rgate', 'dalpha'), impl.rgate_dalpha(dy, x, alpha), *bref['dalpha'])


# ---------------------------------------------------------------- KL
def KL(rid, M, B, Z, prior, pp=0, zero=None, need_prior=True, lv_wide=False):
    """prior: None | 'row' ((M, Z), broadcast over the batch) | 'sample' ((M, B, Z)); pp: columns behind every prior row (ldp_m | ldp_b = Z + pp)"""
    return pytest.param(dict(M=M, B=B, Z=Z, prior=prior, pp=pp, zero=zero, need_prior=need_prior, lv_wide=lv_wide), id=rid)


KL_ROWS = [
    KL('kl M1 B1 Z1 standard', 1, 1, 1, None), KL('kl M2 B3 Z16 row prior', 2, 3, 16, 'row'), KL('kl M3 B17 Z5 row prior contrast 1 weightless', 3, 17, 5, 'row', zero=1),
    KL('kl M8 B5 Z16 row prior ldp_m Z+3', KL_MAXM, 5, 16, 'row', pp=3), KL('kl M2 B5 Z7 sample prior ldp_b Z+3', 2, 5, 7, 'sample', pp=3),
    KL('kl M4 B257 Z16 row prior need_prior false', 4, 257, 16, 'row', need_prior=False), KL('kl M4 B33 Z16 standard lv to +-20', 4, 33, 16, None, lv_wide=True),
    KL('kl M2 B65537 Z16 row prior backward over the grid cap', 2, 65537, 16, 'row'),
]


@functools.lru_cache(maxsize=2)
def kl_case(M, B, Z, prior, zero, lv_wide):
    mu, lv = rnd((M, B, Z), 1), rnd((M, B, Z), 2, 0.7)
    if lv_wide:
        lv.view(-1)[:10] = torch.tensor([-20.0, -5.0, 5.0, 10.0, 20.0] * 2)
        lv[-1, -1, -5:] = torch.tensor([-20.0, -5.0, 5.0, 10.0, 20.0])
    mask = (torch.rand(B, M, generator=torch.Generator().manual_seed(3)) > 0.3).float()
    mask[::2] = 1.0
    if zero is not None:
        mask[:, zero] = 0.0
    w = torch.zeros(M, B)
    for i in range(M):          # the mask and the reference's normalisation, as the caller's host code forms the table
        n = float(mask[:, i].sum())
        if n > 0:
            w[i] = mask[:, i] / (M * n)
    if B > 1:
        w[0, B - 1] = 0.0          # a zero-weight row of a present contrast
    pm = plv = None
    if prior is not None:
        shape = (M, Z) if prior == 'row' else (M, B, Z)
        pm, plv = rnd(shape, 4), rnd(shape, 5, 0.5)
    return dict(mu=mu, lv=lv, w=w, pm=pm, plv=plv)


def row_kl(row, impl, rec):
    M, B, Z = row['M'], row['B'], row['Z']
    c = dict(kl_case(M, B, Z, row['prior'], row['zero'], row['lv_wide']), pp=row['pp'], need_prior=row['need_prior'])
    ref = AT.kl_ref(c['mu'], c['lv'], c['w'], c['pm'], c['plv'], G_UP)
    for lay in (DENSE, (2, 3)):
        tag = ' ' + lay_tag(lay)
        o = impl.kl(c, lay)
        assert ('dpmu' in o) == (row['prior'] is not None and row['need_prior'])
        for n in ('loss', 'dmu', 'dlv', 'dpmu', 'dplv'):
            if n in o:
                rec(n + tag, ('kl', n), o[n], *ref[n])
        if row['zero'] is not None:
            for n in ('dmu', 'dlv', 'dpmu', 'dplv'):
                if n in o:
                    is_zero(o[n][row['zero']], f'{n} of the weightless contrast')
        if B > 1:
            is_zero(o['dmu'][0, B - 1], 'dmu of a zero-weight row'); is_zero(o['dlv'][0, B - 1], 'dlv of a zero-weight row')


# ---------------------------------------------------------------- mean compaction
AVGPOOL_ROWS = [pytest.param(dict(N=N, C=Cc, H=H, W=W, k=k), id=f'avgpool k{k} {N}x{Cc}x{H}x{W}')
                for N, Cc, H, W, k in [(2, 4, 37, 50, 16), (1, 5, 20, 33, 4), (2, 4, 16, 16, 16), (2, 3, 9, 7, 1), (2, 4, 512, 513, 16)]]


def row_avgpool(row, impl, rec):
    N, C, H, W, k = (row[n] for n in ('N', 'C', 'H', 'W', 'k'))
    Ho, Wo = H // k, W // k
    x, dy = rnd((N, H, W, C), 31), rnd((N, C * Ho * Wo), 32)
    x[:, :, :, 0] *= 1e-6
    fref, bref = AT.avgpool_ref(x, k), AT.avgpool_bwd_ref(dy, (N, H, W, C), k)
    for lay in (DENSE, SLICE if C % 4 == 0 else (1, 2)):
        tag = ' ' + lay_tag(lay)
        y = impl.avgpool_fwd(x, k, lay)
        rec('y' + tag, ('avgpool', 'y'), y, *fref)
        dx = impl.avgpool_bwd(dy, (N, H, W, C), k, lay)
        rec('dx' + tag, ('avgpool', 'dx'), dx, *bref)
        is_zero(dx[:, Ho * k:], 'dx in the floor remainder'); is_zero(dx[:, :, Wo * k:], 'dx in the floor remainder')
        if k == 1:          # copies, to the bit
            bits_eq(y, x.permute(0, 3, 1, 2).reshape(N, -1), 'avgpool k = 1 forward'); bits_eq(dx, dy.reshape(N, C, H, W).permute(0, 2, 3, 1), 'avgpool k = 1 backward')


def row_refusals(row, impl, rec):
    res = impl.refusals()
    if res is not None:
        bad = [r for r in res if r[1] != r[2] or r[3]]
        assert not bad, bad
        assert len(res) > 90


# family of the launch counters -> (row function, rows)
OPS = dict(chatt=(row_chatt, CHATT_ROWS), symdiff=(row_symdiff, SYMDIFF_ROWS), rgate=(row_rgate, RGATE_ROWS), kl=(row_kl, KL_ROWS), avgpool=(row_avgpool, AVGPOOL_ROWS),
           refusals=(row_refusals, [pytest.param({}, id='refused arguments launch nothing and write nothing')]))
ALL_ROWS = [pytest.param(op, p.values[0], id=p.id) for op, (_, rows) in OPS.items() for p in rows]


def run_row(op, row, impl, rid, enforce):
    rec = Rec(rid, enforce)
    OPS[op][0](row, impl, rec)
    return rec.items


@pytest.mark.parametrize('op,row', ALL_ROWS)
def test_attn_path(mrdis, request, op, row):
    rid = request.node.callspec.id
    items = run_row(op, row, HipImpl(mrdis), rid, enforce=not MEASURING)
    if MEASURING:
        yard = {name: r for name, _, r in run_row(op, row, TorchImpl(), rid, False)}
        for name, key, r in items:
            dump_measured('attn_path_margins.jsonl', dict(row=rid, out=name, key=list(key), kernel=r, yardstick=yard.get(name), kappa=AT.KAPPA.get(key)))
        for name, key, r in items:
            assert key in AT.KAPPA and r <= AT.KAPPA[key], f'{rid}: {name} needs kappa {r:.2f}, committed {AT.KAPPA.get(key)}'


def test_table_covers_every_family(mrdis):
    """every family of hip.OUTDEC_FAMILIES + hip.LATENT_FAMILIES is the family of a row (HipImpl.call asserts it per call), and every kappa belongs to one"""
    hip = mrdis.hip
    fams = {op for op, (_, rows) in OPS.items() if op != 'refusals' and rows}
    assert fams == set(hip.OUTDEC_FAMILIES + hip.LATENT_FAMILIES), fams ^ set(hip.OUTDEC_FAMILIES + hip.LATENT_FAMILIES)
    assert {k[0] for k in AT.KAPPA} == fams
    assert all(NOT_IN_TABLE.values())
