"""Every branch of the CondConv expert-mix kernels (csrc/mrdis_conv.hip: mix_fwd / mix_routed_fwd / mix_fwd_body, mix_bwd / mix_bwd_body /
mix_bwd_tiled<1|9|16>, the finalize kernels, the all-layers job table), of the optimizer arena (sumsq_finite, adam_advance / adam) and of the helper
kernels the elem-paths suite left out (softmax_mask_drop, recon_err, maxpool, cast_view, slice_gather; csrc/mrdis_elem.hip), element by element
against float64 (tests/aux_check.py).

One row = one entry point, one option set, one geometry.  A row is a function of an implementation object: HipImpl runs the kernels (through
hip.load() where the row chooses leading dimensions, pointers or workspaces, through the hip.py wrappers where it does not), TorchImpl evaluates the
same operation in plain fp32 torch on the CPU -- the yardstick.  tests/test_aux_check.py runs every row with TorchImpl (no GPU) and holds
aux_check.KAPPA to 4 x the worst yardstick ratio; the tests below run them with HipImpl under that table.  Every row with a pitch runs twice:
dense, and through channel or column slices of wider buffers prefilled with NaN, whose neighbouring elements must keep their NaN bits.

Which mix-backward body runs (tiled or element-wise) is decided on the device from (E, M, T) alone and no counter sees it: every mix row states its
side of mix_tiled_ok, asserted against MIXT_E / MIXT_M read out of the source, and every tiled row is run again as MIXT_M + 1 types whose added
gradients are NULL -- the element-wise body -- where dW must have the same bits (the kernel's stated contract).

MRDIS_DUMP_MEASURED=<dir> records both ratios of every row (aux_path_margins.jsonl; profiles/aux_path_margins.txt)."""
import ctypes as C_
import functools
import os
import re

import pytest
import torch

import aux_check as AC
from fixtures import dump_measured

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
B16, F32 = torch.bfloat16, torch.float32
MEASURING = bool(os.environ.get('MRDIS_DUMP_MEASURED'))
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'representation-disentanglement_amd', 'csrc')
_CONV, _ELEM = (open(os.path.join(CSRC, f)).read() for f in ('mrdis_conv.hip', 'mrdis_elem.hip'))
MIXT_E, MIXT_M = (int(x) for x in re.search(r'constexpr int MIXT_E = (\d+), MIXT_M = (\d+)', _CONV).groups())
MIX_MAX_TYPES = int(re.search(r'#define MIX_MAX_TYPES (\d+)', _CONV).group(1))
ADAM_MAX_GATES, SM_MAXC, SUMSQ_BLOCKS = (int(re.search(r'#define %s (\d+)' % n, _ELEM).group(1)) for n in ('ADAM_MAX_GATES', 'SM_MAXC', 'SUMSQ_BLOCKS'))
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
PAD = 8          # elements on each side of a slice (keeps 16-byte alignment)


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
    AC.assert_same_bits(a.detach().cpu().contiguous(), b.detach().cpu().contiguous(), what)


def int_eq(a, b, what):
    a, b = a.detach().cpu(), b.detach().cpu()
    assert a.shape == b.shape and bool((a == b).all()), f'{what}: {int((a != b).sum())} of {a.numel()} differ'


class Rec:
    """collects (output, kappa key, ratio) of one row; enforce: every output is held to its committed kappa"""

    def __init__(self, rid, enforce):
        self.rid, self.enforce, self.items = rid, enforce, []

    def __call__(self, name, key, got, ref, A, u_out=0.0, extra=None):
        if self.enforce:
            assert key in AC.KAPPA, f'no kappa committed for {key}'
            r = AC.check(got, ref, A, AC.KAPPA[key], u_out=u_out, extra=extra, what=f'{self.rid}: {name}')
        else:
            r = AC.ratio(got, ref, A, u_out, extra)
        self.items.append((name, key, r))


# ================================================================ implementations
def is_nan_bits(t, what):
    it = torch.int32 if t.dtype is F32 else torch.int16
    nan = torch.full((1,), float('nan'), dtype=t.dtype).view(it).item()
    assert bool((t.contiguous().view(it) == nan).all()), f'{what}: a store landed outside the output slice'


def w5(W):
    """(E, Co, Ci, T) -> the (E, Co, Ci, kh, kw) the wrappers take"""
    return W.reshape(*W.shape, 1)


class TorchImpl:
    """plain fp32 torch on the CPU: the yardstick.  Layout modes do not apply (there is one dense evaluation)"""
    gpu = False

    # ---- mix
    def mix_fwd(self, c, mode='dense'):
        r = torch.sigmoid(c['types'] @ c['fcw'].T + c['fcb'])
        w = torch.einsum('me,eoct->moct', r, c['W'])
        tck, tkc = [AC.to_tck(x) for x in w], [AC.to_tkc(x) for x in w]
        return dict(r=r, tck=tck, tkc=tkc, btck=[x.to(B16) for x in tck], btkc=[x.to(B16) for x in tkc])

    def mix_bwd(self, c, f, mode='dense'):
        g = AC.mix_routing_grad_ref(c['W'], c['fcw'], c['fcb'], c['types'], c['dws'], dtype=F32)
        out = dict(dW=g['dW'], dfcw=g['dfcw'][0], dfcb=g['dfcb'][0])
        if mode == 'sinks':
            out = {k: c['sinks0'][k] + v for k, v in out.items()}
        return out

    def mix1_fwd(self, W, r):
        w = torch.einsum('e,eoct->oct', r, W)
        return AC.to_tck(w), AC.to_tkc(w)

    def mix1_bwd(self, dw, W, r, dr0):
        g = AC.from_tck(dw)
        return r[:, None, None, None] * g[None], dr0 + (g[None] * W).sum((1, 2, 3))

    def routed_fwd(self, c):
        f = self.mix_fwd(c)
        return dict(r=f['r'][0], tck=f['tck'][0], tkc=f['tkc'][0])

    def routed_bwd(self, c, f):
        return self.mix_bwd(c, f)

    def mix_jobs(self, cases, modes):
        outs = []
        for c, mode in zip(cases, modes):
            f = self.mix_fwd(c)
            f.update(self.mix_bwd(c, f, 'sinks' if mode == 'acc' else 'dense'))
            outs.append(f)
        return outs

    def mix_limits(self):
        return None

    # ---- optimizer
    def sumsq(self, g, out0):
        fin = torch.isfinite(g)
        return torch.tensor(out0[0], dtype=F32) + (g[fin] ** 2).sum(), float(torch.tensor(out0[1], dtype=F32) + (~fin).sum())

    def adam(self, s, host_step=False):
        o = AC.adam_ref(s['p0'], s['grads'], s['flags'], s['ranges'], s['fidx'], clip=s['norm'], dtype=F32, arena_count=not s['own_counts'], **s['hyper'])
        return dict(p=o['p'][0].float(), m=o['m'][0].float(), v=o['v'][0].float(), vmax=o['vmax'][0].float(), applied=o['applied'], skipped=o['skipped'],
                    gate_steps=o['gate_steps'], skip_snaps=[])

    def adam_limits(self):
        return None

    # ---- helpers
    def softmax_fwd(self, s, mask, scale, pad):
        return AC.softmax_md_ref(s, mask, scale, dtype=F32)[0]

    def softmax_bwd(self, dout, out, pad):
        return out * (dout - (out * dout).sum(1, keepdim=True))

    def softmax_limits(self):
        return None

    def recon_fwd(self, gt, x, p, pad):
        d = (gt - x).reshape(gt.shape[0], -1)
        return d.abs().mean(1) if p == 1 else (d * d).mean(1)

    def recon_bwd(self, gt, x, w, p, pad):
        xr = x.clone().requires_grad_(True)
        d = (gt - xr).reshape(gt.shape[0], -1)
        e = d.abs().mean(1) if p == 1 else (d * d).mean(1)
        return torch.autograd.grad((e * w).sum(), xr)[0]

    def maxpool_fwd(self, x, k, pad):
        return AC.maxpool_ref(x, k)

    def maxpool_bwd(self, dy, arg, shape, k, pad):
        return AC.maxpool_bwd_ref(dy, arg, shape)

    def cast_view(self, x, dtype, Cd, mode, v1):
        return AC.cast_view_ref(x, dtype, Cd)

    def slice_gather(self, vols, slice_idx, drop, H, W, D, block, ld_extra):
        return AC.slice_gather_ref(vols, slice_idx, drop, H, W, D, block)

    def slice_gather_limits(self):
        return None


def d_(t):
    return t.to(DEV).contiguous()


def ptr_array(ts, off_bytes=0):
    return (C_.c_void_p * len(ts))(*[None if t is None else t.data_ptr() + off_bytes for t in ts])


class HipImpl:
    """the kernels under test.  mode 'fused' / pad > 0: operands are slices of wider buffers (random or NaN beside them), results land in slices of
    NaN-prefilled buffers whose neighbours are checked here"""
    gpu = True
    COL0, EXTRA = 3, 5          # a fused-half run writes / reads columns [3, 3 + Co) of Co + 5

    def __init__(self, m):
        self.hip, self.lib = m.hip, m.hip.load()

    def st(self):
        return self.hip._stream()

    # ---- mix
    def mix_fwd(self, c, mode='dense'):
        hip = self.hip
        W, fcw, fcb, types = (d_(c[k]) for k in ('W', 'fcw', 'fcb', 'types'))
        E, Co, Ci, T = c['W'].shape
        M = types.shape[0]
        if mode == 'dense':
            tck, tkc, r, btck, btkc = hip.mix_experts_routed_multi_fwd(w5(W), fcw, fcb, types, want_bf16=True)
        else:
            col0, cot = self.COL0, Co + self.EXTRA
            mk = lambda shape, dt: [torch.full(shape, float('nan'), dtype=dt, device=DEV) for _ in range(M)]
            wt, wk, bt, bk = mk((T, Ci, cot), F32), mk((T, cot, Ci), F32), mk((T, Ci, cot), B16), mk((T, cot, Ci), B16)
            r = hip.mix_experts_routed_multi_fwd(w5(W), fcw, fcb, types, into=(wt, wk, bt, bk, col0, cot))
            for m in range(M):
                for t in (wt[m], bt[m]):
                    is_nan_bits(t[:, :, :col0], 'tck'); is_nan_bits(t[:, :, col0 + Co:], 'tck')
                for t in (wk[m], bk[m]):
                    is_nan_bits(t[:, :col0], 'tkc'); is_nan_bits(t[:, col0 + Co:], 'tkc')
            tck, btck = [t[:, :, col0:col0 + Co] for t in wt], [t[:, :, col0:col0 + Co] for t in bt]
            tkc, btkc = [t[:, col0:col0 + Co] for t in wk], [t[:, col0:col0 + Co] for t in bk]
        cp = lambda ts: [t.cpu().contiguous() for t in ts]
        return dict(r=r.cpu(), r_dev=r, tck=cp(tck), tkc=cp(tkc), btck=cp(btck), btkc=cp(btkc))

    def mix_bwd(self, c, f, mode='dense'):
        hip = self.hip
        W, types = d_(c['W']), d_(c['types'])
        E, Co, Ci, T = c['W'].shape
        kw = {}
        if mode == 'fused':          # the gradients are a column block of wider tensors; NaN beside them: reading a neighbour poisons the result
            col0, ld = self.COL0, Co + self.EXTRA
            dws = []
            for g in c['dws']:
                if g is None:
                    dws.append(None)
                    continue
                wide = torch.full((T, Ci, ld), float('nan'), device=DEV)
                wide[:, :, col0:col0 + Co] = d_(g)
                dws.append(wide)
            kw = dict(col0=col0, ld=ld)
        else:
            dws = [None if g is None else d_(g) for g in c['dws']]
        if mode == 'sinks':
            kw = dict(sinks=tuple(d_(c['sinks0'][k]) for k in ('dW', 'dfcw', 'dfcb')))
        dW, dfcw, dfcb = hip.mix_experts_routed_multi_bwd(dws, w5(W), f['r_dev'], types, **kw)
        return dict(dW=dW.reshape(E, Co, Ci, T).cpu(), dfcw=dfcw.cpu(), dfcb=dfcb.cpu())

    def mix1_fwd(self, W, r):
        tck, tkc = self.hip.mix_experts_fwd(w5(d_(W)), d_(r))
        return tck.cpu(), tkc.cpu()

    def mix1_bwd(self, dw, W, r, dr0):
        lib = self.lib
        E, Co, Ci, T = W.shape
        Wd, rd, g, dr = d_(W), d_(r), d_(dw), d_(dr0)
        dW = torch.full((E, Co, Ci, T), float('nan'), device=DEV)
        nb = lib.mrdis_mix_experts_bwd_workspace(E, Co, Ci, T)
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV)
        assert lib.mrdis_mix_experts_bwd(g.data_ptr(), Wd.data_ptr(), rd.data_ptr(), dW.data_ptr(), dr.data_ptr(), ws.data_ptr(), nb - 1, E, Co, Ci, T, self.st()) == EWORKSPACE
        rc = lib.mrdis_mix_experts_bwd(g.data_ptr(), Wd.data_ptr(), rd.data_ptr(), dW.data_ptr(), dr.data_ptr(), ws.data_ptr(), nb, E, Co, Ci, T, self.st())
        assert rc == 0, rc
        return dW.cpu(), dr.cpu()

    def routed_fwd(self, c):
        tck, tkc, r = self.hip.mix_experts_routed_fwd(w5(d_(c['W'])), d_(c['fcw']), d_(c['fcb']), d_(c['types']))
        return dict(r=r.cpu(), r_dev=r, tck=tck.cpu(), tkc=tkc.cpu())

    def routed_bwd(self, c, f):
        E, Co, Ci, T = c['W'].shape
        dW, dfcw, dfcb = self.hip.mix_experts_routed_bwd(d_(c['dws'][0]), w5(d_(c['W'])), f['r_dev'], d_(c['types']), c['fcw'].shape[1])
        return dict(dW=dW.reshape(E, Co, Ci, T).cpu(), dfcw=dfcw.cpu(), dfcb=dfcb.cpu())

    def mix_jobs(self, cases, modes):
        """one job per case.  modes: 'plain' | 'padded' (ci_pitch 16 > Ci into zeroed buffers) | 'fused' (a column block of wider NaN-prefilled
        filters, gradients a column block of wider tensors) | 'acc' (accumulate into the prefilled sinks c['sinks0'])"""
        hip = self.hip
        types = d_(cases[0]['types'])
        M = types.shape[0]
        jobs, keep, blocks = [], [], 0
        dwtab = torch.zeros(len(cases), 8, dtype=torch.int64)
        for k, (c, mode) in enumerate(zip(cases, modes)):
            E, Co, Ci, T = c['W'].shape
            cip = 16 if mode == 'padded' else Ci
            ld, col0 = (Co + self.EXTRA, self.COL0) if mode == 'fused' else (Co, 0)
            fill = 0.0 if mode == 'padded' else float('nan')
            W, fcw, fcb = d_(c['W']), d_(c['fcw']), d_(c['fcb'])
            r = torch.zeros(M * E, device=DEV)
            tck = [torch.full((T, cip, ld), fill, device=DEV) for _ in range(M)]; tkc = [torch.full((T, ld, cip), fill, device=DEV) for _ in range(M)]
            btck = [torch.full((T, cip, ld), fill, dtype=B16, device=DEV) for _ in range(M)]; btkc = [torch.full((T, ld, cip), fill, dtype=B16, device=DEV) for _ in range(M)]
            if mode == 'acc':
                sinks = [d_(c['sinks0'][n]) for n in ('dW', 'dfcw', 'dfcb')]
            else:
                sinks = [torch.full(c[n].shape, float('nan'), device=DEV) for n in ('W', 'fcw', 'fcb')]
            nblk = hip.mix_job_blocks(Co, Ci, T)
            part = torch.empty(8 * nblk * M, device=DEV)
            dws = []
            for m, g in enumerate(c['dws']):
                if g is None:
                    dws.append(None)
                    continue
                wide = torch.full((T, cip, ld), float('nan'), device=DEV)
                wide[:, :Ci, col0:col0 + Co] = d_(g)
                dws.append(wide); dwtab[k, m] = wide.data_ptr() + 4 * col0
            j = hip.MixJob()
            j.W, j.fcw, j.fcb, j.r = W.data_ptr(), fcw.data_ptr(), fcb.data_ptr(), r.data_ptr()
            for m in range(M):
                j.tck[m], j.tkc[m] = tck[m].data_ptr() + 4 * col0, tkc[m].data_ptr() + 4 * col0 * cip
                j.btck[m], j.btkc[m] = btck[m].data_ptr() + 2 * col0, btkc[m].data_ptr() + 2 * col0 * cip
            j.dW, j.dfcw, j.dfcb, j.part = sinks[0].data_ptr(), sinks[1].data_ptr(), sinks[2].data_ptr(), part.data_ptr()
            j.tap_tkc = ld * cip
            j.E, j.Co, j.Ci, j.T, j.ld_tck, j.ld_dw = E, Co, Ci, T, ld, ld
            j.block0, j.nblk, j.accumulate, j.ci_pitch = blocks, nblk, 1 if mode == 'acc' else 0, cip
            blocks += nblk
            jobs.append(j); keep.append((W, fcw, fcb, r, tck, tkc, btck, btkc, sinks, part, dws))
        table = hip.mix_job_table(jobs, DEV)
        hip.mix_jobs_fwd(table, len(jobs), blocks, types)
        dtab = d_(dwtab)
        hip.mix_jobs_bwd(table, len(jobs), blocks, dtab, types)
        torch.cuda.synchronize()
        outs = []
        for (c, mode), (W, fcw, fcb, r, tck, tkc, btck, btkc, sinks, part, dws) in zip(zip(cases, modes), keep):
            E, Co, Ci, T = c['W'].shape
            col0 = self.COL0 if mode == 'fused' else 0
            for m in range(M):
                for a, b in ((tck[m], tkc[m]), (btck[m], btkc[m])):
                    if mode == 'padded':          # the padding channels stay zero
                        assert not bool(a[:, Ci:].any()) and not bool(b[:, :, Ci:].any()), 'a store landed in the zero padding of a padded filter'
                    elif mode == 'fused':
                        for side in (a[:, :, :col0], a[:, :, col0 + Co:], b[:, :col0], b[:, col0 + Co:]):
                            is_nan_bits(side, 'fused job')
            cp = lambda ts, f: [f(t).cpu().contiguous() for t in ts]
            outs.append(dict(r=r.reshape(M, E).cpu(), tck=cp(tck, lambda t: t[:, :Ci, col0:col0 + Co]), tkc=cp(tkc, lambda t: t[:, col0:col0 + Co, :Ci]),
                             btck=cp(btck, lambda t: t[:, :Ci, col0:col0 + Co]), btkc=cp(btkc, lambda t: t[:, col0:col0 + Co, :Ci]),
                             dW=sinks[0].cpu(), dfcw=sinks[1].cpu(), dfcb=sinks[2].cpu()))
        return outs

    def mix_limits(self):
        """E = 9, M = 9 and emb = 17 are refused before anything is launched; so is a short workspace"""
        lib, st = self.lib, self.st()
        W = torch.zeros(9 * 4 * 4 * 9, device=DEV); v = torch.zeros(9 * 17, device=DEV); ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
        outs = [torch.zeros(4 * 4 * 9, device=DEV) for _ in range(9)]
        p = lambda t: t.data_ptr()
        fwd = lambda E, M, emb: lib.mrdis_mix_experts_routed_multi_fwd(p(W), p(v), p(v), p(v), emb, M, p(v), ptr_array(outs[:M]), ptr_array(outs[:M]), None, None, 0, 0, E, 4, 4, 9, st)
        bwd = lambda E, M, emb, nb: lib.mrdis_mix_experts_routed_multi_bwd(ptr_array(outs[:M]), p(W), p(v), p(v), emb, M, p(W), p(v), p(v), 0, 0, p(ws), nb, E, 4, 4, 9, st)
        need = lib.mrdis_mix_experts_routed_multi_bwd_workspace(4, 3, 4, 4, 9)
        got = dict(fwd_E9=fwd(9, 4, 1), fwd_M9=fwd(3, MIX_MAX_TYPES + 1, 1), fwd_emb17=fwd(3, 4, 17), bwd_E9=bwd(9, 4, 1, 4096), bwd_M9=bwd(3, MIX_MAX_TYPES + 1, 1, 4096),
                   bwd_emb17=bwd(3, 4, 17, 4096), bwd_short=bwd(3, 4, 1, need - 1),
                   r_fwd_E9=lib.mrdis_mix_experts_routed_fwd(p(W), p(v), p(v), p(v), 1, p(v), p(outs[0]), p(outs[1]), 9, 4, 4, 9, st),
                   r_fwd_emb17=lib.mrdis_mix_experts_routed_fwd(p(W), p(v), p(v), p(v), 17, p(v), p(outs[0]), p(outs[1]), 3, 4, 4, 9, st),
                   r_bwd_short=lib.mrdis_mix_experts_routed_bwd(p(outs[0]), p(W), p(v), p(v), 1, p(W), p(v), p(v), p(ws), lib.mrdis_mix_experts_bwd_workspace(3, 4, 4, 9) - 1, 3, 4, 4, 9, st),
                   fwd1_E9=lib.mrdis_mix_experts_fwd(p(W), p(v), p(outs[0]), p(outs[1]), 9, 4, 4, 9, st))
        want = {k: (EWORKSPACE if k.endswith('short') else EINVAL) for k in got}
        return got, want

    # ---- optimizer
    def sumsq(self, g, out0):
        out = torch.tensor(list(out0), dtype=F32, device=DEV)
        self.hip.sumsq_finite(d_(g), out)
        o = out.cpu()
        return o[0], float(o[1])

    def adam(self, s, host_step=False):
        hip, h = self.hip, s['hyper']
        n = s['p0'].numel()
        p = d_(s['p0']); m, v, vm = (torch.zeros(n, device=DEV) for _ in range(3))
        nf = torch.zeros(2, device=DEV) if s['norm'] else None
        state = None if host_step else torch.zeros(2, device=DEV)
        n_flags = (max(s['fidx']) + 1) if s['fidx'] else 0
        gsteps = torch.zeros(3 * n_flags, device=DEV) if n_flags and s['own_counts'] and not host_step else None
        ng = n_flags if gsteps is not None else 0
        snaps, applied = [], 0
        for k, g in enumerate(s['grads']):
            gd = d_(g)
            if nf is not None:
                nf.zero_(); hip.sumsq_finite(gd, nf)
            gates = (s['ranges'], s['fidx'], torch.tensor([float(x) for x in s['flags'][k]], device=DEV)) if n_flags else None
            skip = s['norm'] and not bool(torch.isfinite(g).all())
            before = [t.clone() for t in (p, m, v, vm)] + ([gsteps[:ng].clone()] if ng else [])
            applied += 0 if skip else 1          # (a caller's host counter does not advance over a skipped step)
            hip.adam_amsgrad_step(p, gd, m, v, vm, h['lr'], h['b1'], h['b2'], h['eps'], h['wd'], max(applied, 1), nf, h['max_norm'], h['grad_scale'],
                                  step_state=state, gates=gates, gate_steps=gsteps)
            if skip:
                snaps.append((before, [t.clone() for t in (p, m, v, vm)] + ([gsteps[:ng].clone()] if ng else [])))
        st = state.cpu() if state is not None else None
        return dict(p=p.cpu(), m=m.cpu(), v=v.cpu(), vmax=vm.cpu(), applied=None if st is None else float(st[0]), skipped=None if st is None else float(st[1]),
                    gate_steps=[float(x) for x in gsteps[:ng].cpu()] if ng else [], skip_snaps=snaps)

    def adam_limits(self):
        """ADAM_MAX_GATES ranges are accepted, one more is refused"""
        hip = self.hip
        n = ADAM_MAX_GATES + 8
        bufs = [torch.zeros(n, device=DEV) for _ in range(5)]
        state = torch.zeros(2, device=DEV)
        got = []
        for ng in (ADAM_MAX_GATES, ADAM_MAX_GATES + 1):
            ranges = [(i, i + 1) for i in range(ng)]
            flags = torch.ones(ADAM_MAX_GATES, device=DEV)
            try:
                hip.adam_amsgrad_step(*bufs, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, 0.0, step_state=state, gates=(ranges, [i % ADAM_MAX_GATES for i in range(ng)], flags),
                                      gate_steps=torch.zeros(3 * ADAM_MAX_GATES, device=DEV))
                got.append(0)
            except hip.MrdisError:
                got.append(EINVAL)
        try:          # gate_steps needs step_state
            hip.adam_amsgrad_step(*bufs, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, 0.0, step_state=None, gates=([(0, 1)], [0], torch.ones(1, device=DEV)),
                                  gate_steps=torch.zeros(3, device=DEV))
            got.append(0)
        except hip.MrdisError:
            got.append(EINVAL)
        return got, [0, EINVAL, EINVAL]

    # ---- helpers.  2-D operands (P, C): pad > 0 puts them into (P, C + 2 pad) buffers
    def put(self, t, pad, seed=5):
        t = t.reshape(-1, t.shape[-1])
        if not pad:
            return d_(t)
        P, C = t.shape
        buf = d_(torch.cat([rnd((P, pad), seed), t, rnd((P, pad), seed + 1)], 1).to(t.dtype))
        return buf[:, pad:pad + C]

    def out(self, P, C, pad, dtype=F32):
        buf = torch.full((P, C + 2 * pad), float('nan'), dtype=dtype, device=DEV)
        return buf, buf[:, pad:pad + C]

    def done(self, buf, view, pad, what):
        if pad:
            C = view.shape[1]
            is_nan_bits(buf[:, :pad], what); is_nan_bits(buf[:, pad + C:], what)
        return view.cpu().contiguous()

    def softmax_fwd(self, s, mask, scale, pad):
        P, C = s.shape
        sv = self.put(s, pad); buf, o = self.out(P, C, pad)
        mk = None if mask is None else d_(mask)
        rc = self.lib.mrdis_softmax_mask_drop_fwd(sv.data_ptr(), sv.stride(0), None if mk is None else mk.data_ptr(), o.data_ptr(), o.stride(0), P, C, scale, self.st())
        assert rc == 0, rc
        return self.done(buf, o, pad, 'softmax out')

    def softmax_bwd(self, dout, out, pad):
        P, C = out.shape
        dv, ov = self.put(dout, pad), self.put(out, pad, 7); buf, ds = self.out(P, C, pad)
        rc = self.lib.mrdis_softmax_mask_drop_bwd(dv.data_ptr(), dv.stride(0), ov.data_ptr(), ov.stride(0), ds.data_ptr(), ds.stride(0), P, C, self.st())
        assert rc == 0, rc
        return self.done(buf, ds, pad, 'softmax ds')

    def softmax_limits(self):
        lib, C = self.lib, SM_MAXC + 1
        s = torch.zeros(4, C, device=DEV); o = torch.zeros(4, C, device=DEV)
        got = [lib.mrdis_softmax_mask_drop_fwd(s.data_ptr(), C, None, o.data_ptr(), C, 4, C, 100.0, self.st()),
               lib.mrdis_softmax_mask_drop_bwd(s.data_ptr(), C, s.data_ptr(), C, o.data_ptr(), C, 4, C, self.st())]
        return got, [EUNSUPPORTED, EUNSUPPORTED]

    def recon_fwd(self, gt, x, p, pad):
        N, HW, C = x.shape
        g, xv = self.put(gt, pad), self.put(x, pad, 9)
        out = torch.full((N,), float('nan'), device=DEV)
        nb = self.lib.mrdis_recon_err_workspace(N, HW, C)
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        assert self.lib.mrdis_recon_err_fwd(g.data_ptr(), g.stride(0), xv.data_ptr(), xv.stride(0), out.data_ptr(), ws.data_ptr(), nb - 1, N, HW, C, p, self.st()) == EWORKSPACE
        rc = self.lib.mrdis_recon_err_fwd(g.data_ptr(), g.stride(0), xv.data_ptr(), xv.stride(0), out.data_ptr(), ws.data_ptr(), nb, N, HW, C, p, self.st())
        assert rc == 0, rc
        return out.cpu()

    def recon_bwd(self, gt, x, w, p, pad):
        N, HW, C = x.shape
        g, xv = self.put(gt, pad), self.put(x, pad, 9); buf, dx = self.out(N * HW, C, pad)
        rc = self.lib.mrdis_recon_err_bwd(g.data_ptr(), g.stride(0), xv.data_ptr(), xv.stride(0), d_(w).data_ptr(), dx.data_ptr(), dx.stride(0), N, HW, C, p, self.st())
        assert rc == 0, rc
        return self.done(buf, dx, pad, 'recon dx').reshape(N, HW, C)

    def maxpool_fwd(self, x, k, pad):
        N, C, H, W = x.shape
        xv = self.put(x.permute(0, 2, 3, 1), pad)
        Ho, Wo = H // k, W // k
        y = torch.full((N, Ho, Wo, C), float('nan'), device=DEV); arg = torch.full((N, Ho, Wo, C), -1, dtype=torch.int32, device=DEV)
        rc = self.lib.mrdis_maxpool_fwd(xv.data_ptr(), xv.stride(0), y.data_ptr(), arg.data_ptr(), N, H, W, C, k, self.st())
        assert rc == 0, rc
        return y.permute(0, 3, 1, 2).cpu().contiguous(), arg.permute(0, 3, 1, 2).cpu().contiguous()

    def maxpool_bwd(self, dy, arg, shape, k, pad):
        N, C, H, W = shape
        dyd, ad = d_(dy.permute(0, 2, 3, 1)), d_(arg.permute(0, 2, 3, 1))
        buf, dx = self.out(N * H * W, C, pad)
        rc = self.lib.mrdis_maxpool_bwd(dyd.data_ptr(), ad.data_ptr(), dx.data_ptr(), dx.stride(0), N, H, W, C, k, self.st())
        assert rc == 0, rc
        return self.done(buf, dx, pad, 'maxpool dx').reshape(N, H, W, C).permute(0, 3, 1, 2).contiguous()

    def cast_view(self, x, dtype, Cd, mode, v1):
        """mode: 'dense' | 'slice' (8 channels beside the views: aligned) | 'off1' (one channel beside them: the V = 1 instantiation)"""
        hip = self.hip
        N, Cs, H, W = x.shape
        pad = dict(dense=0, slice=PAD, off1=1)[mode]
        xv = self.put(x.permute(0, 2, 3, 1), pad)
        buf, y = self.out(N * H * W, Cd, pad, dtype)
        dt = lambda t: 2 if t is B16 else 0
        hip.launch_counts(reset=True)
        rc = self.lib.mrdis_cast_view(xv.data_ptr(), xv.stride(0), dt(x.dtype), Cs, y.data_ptr(), y.stride(0), dt(dtype), Cd, N * H * W, self.st())
        assert rc == 0, rc
        cnt = hip.launch_counts(reset=True, elem=True)
        assert cnt['elem_v1'] == (1 if v1 else 0), f"elem_v1 counted {cnt['elem_v1']}, the row expects {'V1' if v1 else 'V4'}"
        return self.done(buf, y, pad, 'cast_view').reshape(N, H, W, Cd).permute(0, 3, 1, 2).contiguous()

    def slice_gather(self, vols, slice_idx, drop, H, W, D, block, ld_extra):
        B, M = len(vols), len(vols[0])
        Cc = M * (2 * block + 1)
        dev = {}
        for row in vols:
            for v in row:
                if v is not None and id(v) not in dev:
                    dev[id(v)] = d_(v)
        ptrs = d_(torch.tensor([[0 if v is None else dev[id(v)].data_ptr() for v in row] for row in vols], dtype=torch.int64))
        si, dr = d_(torch.tensor(slice_idx, dtype=torch.int32)), d_(torch.tensor(drop, dtype=torch.int32))
        buf = torch.full((B * H * W, Cc + ld_extra), float('nan'), device=DEV)
        mask = torch.full((B, M), float('nan'), device=DEV); mimg = torch.full((B, H, W), float('nan'), device=DEV)
        rc = self.lib.mrdis_slice_gather(ptrs.data_ptr(), si.data_ptr(), dr.data_ptr(), buf.data_ptr(), Cc + ld_extra, mask.data_ptr(), mimg.data_ptr(), B, M, H, W, D, block, self.st())
        assert rc == 0, rc
        if ld_extra:
            is_nan_bits(buf[:, Cc:], 'slice_gather inputs')
        return buf[:, :Cc].reshape(B, H, W, Cc).permute(0, 3, 1, 2).cpu().contiguous(), mask.cpu(), mimg.cpu()

    def slice_gather_limits(self):
        z = torch.zeros(16, dtype=torch.int64, device=DEV)
        p = z.data_ptr()
        return [self.lib.mrdis_slice_gather(p, p, p, p, 4, p, p, 65536, 4, 1, 1, 1, 0, self.st())], [EUNSUPPORTED]


# ================================================================ rows
# ---------------------------------------------------------------- expert mixing
@functools.lru_cache(maxsize=None)
def mix_case(E, M, Co, Ci, T, emb=1, present=None, seed=100):
    """W (E, Co, Ci, T), the routing Linear, the type rows ((1 + m) as the model feeds them where emb = 1) and one gradient per present type"""
    present = (True,) * M if present is None else present
    types = (1.0 + torch.arange(M, dtype=F32))[:, None] if emb == 1 else rnd((M, emb), seed + 3, 0.5)
    c = dict(W=rnd((E, Co, Ci, T), seed), fcw=rnd((E, emb), seed + 1, 0.5), fcb=rnd((E,), seed + 2), types=types,
             dws=[rnd((T, Ci, Co), seed + 10 + m) if present[m] else None for m in range(M)])
    c['sinks0'] = dict(dW=rnd((E, Co, Ci, T), seed + 30), dfcw=rnd((E, emb), seed + 31), dfcb=rnd((E,), seed + 32))
    return c


def mix_refs(c):
    r, A_r = AC.routing_ref(c['fcw'], c['fcb'], c['types'])
    w, A_w = AC.mix_fwd_ref(c['W'], r)
    dW, A_dW = AC.mix_dW_ref(c['dws'], r) if any(g is not None for g in c['dws']) else (torch.zeros(c['W'].shape, dtype=torch.float64),) * 2
    g = AC.mix_routing_grad_ref(c['W'], c['fcw'], c['fcb'], c['types'], c['dws'])
    return dict(r=(r, A_r), w=(w, A_w), dW=(dW, A_dW), dfcw=g['dfcw'], dfcb=g['dfcb'])


def rec_fwd(rec, f, ref, tag=''):
    rec('r' + tag, ('mix', 'r'), f['r'], *ref['r'])
    for m in range(len(f['tck'])):
        rec(f'w[{m}]' + tag, ('mix', 'w'), f['tck'][m], AC.to_tck(ref['w'][0][m]), AC.to_tck(ref['w'][1][m]))
        bits_eq(f['tkc'][m], f['tck'][m].transpose(1, 2), f'tkc[{m}] against tck[{m}] transposed' + tag)
        if 'btck' in f:
            bits_eq(f['btck'][m], f['tck'][m].to(B16), f'bf16 tck[{m}]' + tag); bits_eq(f['btkc'][m], f['tkc'][m].to(B16), f'bf16 tkc[{m}]' + tag)


def rec_bwd(rec, b, ref, tag=''):
    for n in ('dW', 'dfcw', 'dfcb'):
        rec(n + tag, ('mix', n), b[n], *ref[n])


def tiled_ok(E, M, T):
    return E <= MIXT_E and M <= MIXT_M and T in (1, 9, 16)


def MX(rid, E, M, Co, Ci, T, tiled, present=None, emb=1):
    return pytest.param(dict(E=E, M=M, Co=Co, Ci=Ci, T=T, tiled=tiled, present=present, emb=emb), id=rid)


MIX_ROWS = [
    # ---- tiled (E <= MIXT_E, M <= MIXT_M, T in 1 | 9 | 16)
    MX('tiled T9 33x9 cout and channel tile tails', 3, 4, 33, 9, 9, True),
    MX('tiled T9 32x8 one exact tile', 3, 1, 32, 8, 9, True),
    MX('tiled T9 256x136 136 tiles over 128 blocks parity flips', 3, 3, 256, 136, 9, True),
    MX('tiled T1 33x9 2 blocks 4 tiles 3 of 4 gradients', 3, 4, 33, 9, 1, True, present=(True, False, True, True)),
    MX('tiled T16 40x12 two passes of 8 taps', 3, 4, 40, 12, 16, True),
    MX('tiled T16 7x4 E2 M2', 2, 2, 7, 4, 16, True),
    MX('tiled T9 only m0 present', 3, 4, 33, 9, 9, True, present=(True, False, False, False)),
    MX('tiled T9 m0 absent', 3, 4, 33, 9, 9, True, present=(False, True, True, True)),
    MX('tiled T9 all but one absent', 3, 4, 33, 9, 9, True, present=(False, False, True, False)),
    MX('tiled T9 emb16', 3, 2, 33, 9, 9, True, emb=16),
    # ---- element-wise
    MX('elementwise E4', 4, 2, 40, 24, 9, False),
    MX('elementwise M5', 3, 5, 40, 24, 9, False),
    MX('elementwise E8 M8', 8, 8, 5, 3, 9, False),
    MX('elementwise T4', 3, 4, 9, 5, 4, False),
    MX('elementwise T25', 3, 4, 9, 5, 25, False),
    MX('elementwise m0 absent', 3, 5, 9, 5, 9, False, present=(False, True, False, True, True)),
]


def row_mix(row, impl, rec):
    E, M, Co, Ci, T = (row[k] for k in ('E', 'M', 'Co', 'Ci', 'T'))
    assert row['tiled'] == tiled_ok(E, M, T), 'the row states the wrong side of mix_tiled_ok'
    c = mix_case(E, M, Co, Ci, T, row['emb'], row['present'])
    ref = mix_refs(c)
    dense = None
    for mode in ('dense', 'fused'):
        f = impl.mix_fwd(c, mode)
        rec_fwd(rec, f, ref, ' ' + mode)
        b = impl.mix_bwd(c, f, mode)
        rec_bwd(rec, b, ref, ' ' + mode)
        if dense is None:
            dense, fd = b, f
        else:          # the column-block run reads and sums the same values in the same order
            bits_eq(b['dW'], dense['dW'], 'dW fused half against dense')
    s = impl.mix_bwd(c, fd, 'sinks')
    for n in ('dW', 'dfcw', 'dfcb'):          # accumulate: sink + the non-accumulated result, added in fp32
        bits_eq(s[n], c['sinks0'][n] + dense[n], f'{n} accumulated into a prefilled sink')
    if row['tiled']:          # the same data as MIXT_M + 1 types, the added ones without gradient: the element-wise body
        M2 = MIXT_M + 1
        c2 = dict(c)
        c2['types'] = torch.cat([c['types'], c['types'][-1:].expand(M2 - M, -1) + 0.5])
        c2['dws'] = list(c['dws']) + [None] * (M2 - M)
        assert not tiled_ok(E, M2, T)
        f2 = impl.mix_fwd(c2, 'dense')
        bits_eq(f2['r'][:M], fd['r'], 'r of the first M types')
        b2 = impl.mix_bwd(c2, f2, 'dense')
        bits_eq(b2['dW'], dense['dW'], 'dW tiled against element-wise')
        rec('dfcw elementwise twin', ('mix', 'dfcw'), b2['dfcw'], *ref['dfcw']); rec('dfcb elementwise twin', ('mix', 'dfcb'), b2['dfcb'], *ref['dfcb'])


MIX1_ROWS = [pytest.param(dict(E=3, Co=33, Ci=9, T=9, emb=1), id='single E3 33x9 T9 emb1'), pytest.param(dict(E=3, Co=33, Ci=9, T=9, emb=16), id='single E3 33x9 T9 emb16'),
             pytest.param(dict(E=8, Co=5, Ci=3, T=16, emb=1), id='single E8 5x3 T16 emb1'), pytest.param(dict(E=8, Co=5, Ci=3, T=16, emb=16), id='single E8 5x3 T16 emb16')]


def row_mix1(row, impl, rec):
    """the single-type entry points: mrdis_mix_experts_fwd / _bwd (r given; _bwd ADDS into dr) and mrdis_mix_experts_routed_fwd / _bwd"""
    E, Co, Ci, T, emb = (row[k] for k in ('E', 'Co', 'Ci', 'T', 'emb'))
    c = mix_case(E, 1, Co, Ci, T, emb, None, 300)
    W, dw = c['W'], c['dws'][0]
    r = torch.rand(E, generator=torch.Generator().manual_seed(5)); dr0 = rnd((E,), 6, 10.0)
    tck, tkc = impl.mix1_fwd(W, r)
    w, A = AC.mix_fwd_ref(W, r)
    rec('w (r given)', ('mix1', 'w'), tck, AC.to_tck(w), AC.to_tck(A))
    bits_eq(tkc, tck.transpose(1, 2), 'tkc against tck transposed')
    dW, dr = impl.mix1_bwd(dw, W, r, dr0)
    rec('dW (r given)', ('mix1', 'dW'), dW, *AC.mix_dW_ref([dw], r[None]))
    rec('dr into a prefilled dr', ('mix1', 'dr'), dr, *AC.mix_dr_ref(dw, W, dr0))
    ref = mix_refs(c)
    f = impl.routed_fwd(c)
    rec('r', ('mix', 'r'), f['r'], ref['r'][0][0], ref['r'][1][0])
    rec('w', ('mix', 'w'), f['tck'], AC.to_tck(ref['w'][0][0]), AC.to_tck(ref['w'][1][0]))
    bits_eq(f['tkc'], f['tck'].transpose(1, 2), 'routed tkc against tck transposed')
    rec_bwd(rec, impl.routed_bwd(c, f), ref, ' routed')


def row_mix_jobs(row, impl, rec):
    """the all-layers job table: four jobs (T = 1, 9, 16, 25) in one launch pair, against float64 and against the bits of the per-layer launches"""
    M = 3
    cases = [mix_case(3, M, 33, 9, 1, 1, (True, False, True), 400), mix_case(3, M, 5, 4, 9, 1, None, 410),
             mix_case(3, M, 40, 12, 16, 1, (False, True, True), 420), mix_case(3, M, 9, 5, 25, 1, None, 430)]
    modes = ['plain', 'padded', 'fused', 'acc']
    assert [tiled_ok(3, M, c['W'].shape[3]) for c in cases] == [True, True, True, False]
    outs = impl.mix_jobs(cases, modes)
    for k, (c, mode, o) in enumerate(zip(cases, modes, outs)):
        ref = mix_refs(c)
        tag = f' job {k} {mode}'
        rec_fwd(rec, o, ref, tag)
        f = impl.mix_fwd(c, 'dense')
        b = impl.mix_bwd(c, f, 'dense')
        if mode == 'acc':
            A0 = {n: c['sinks0'][n].double().abs() for n in ('dW', 'dfcw', 'dfcb')}
            for n in ('dW', 'dfcw', 'dfcb'):
                rec(n + tag, ('mix', n), o[n], ref[n][0] + c['sinks0'][n].double(), ref[n][1] + A0[n])
                bits_eq(o[n], c['sinks0'][n] + b[n], n + tag + ' against sink + the per-layer launch')
        else:
            rec_bwd(rec, o, ref, tag)
            for n in ('dW', 'dfcw', 'dfcb'):
                bits_eq(o[n], b[n], n + tag + ' against the per-layer launch')
        bits_eq(o['r'], f['r'], 'r' + tag + ' against the per-layer launch')
        for m in range(M):
            bits_eq(o['tck'][m], f['tck'][m], f'tck[{m}]' + tag + ' against the per-layer launch')


# ---------------------------------------------------------------- optimizer arena
NONFINITE = (float('inf'), float('-inf'), float('nan'))
BIG_N = SUMSQ_BLOCKS * 256 + 3          # every block of the capped grid walks a second stride
SUMSQ_ROWS = [pytest.param(dict(n=n, bad=bad, out0=out0), id=f'sumsq n{n} bad{bad} out0 {out0[0]}')
              for n, bad, out0 in [(1, 0, (0.0, 0.0)), (1, 1, (0.0, 0.0)), (255, 2, (0.0, 0.0)), (257, 0, (3.5, 2.0)), (257, 1, (0.0, 0.0)),
                                   (BIG_N, 300, (1234.5, 7.0)), (BIG_N, 0, (0.0, 0.0))]]


def row_sumsq(row, impl, rec):
    n, bad = row['n'], row['bad']
    g = rnd((n,), 50, 3.0)
    where = torch.randperm(n, generator=torch.Generator().manual_seed(51))[:bad]
    for i, w in enumerate(where):
        g[w] = NONFINITE[i % 3]
    ref, A, cnt = AC.sumsq_ref(g, row['out0'])
    s, c = impl.sumsq(g, row['out0'])
    rec('sum', ('sumsq', 'sum'), s.reshape(1), ref, A)
    assert c == cnt, f'non-finite count {c}, expected {cnt}'


HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-5, max_norm=1.0, grad_scale=1.0)
K_STEPS = 4
PATTERN = [[1, 1], [1, 0], [0, 1], [1, 1]]          # the per-gate step counts (3, 3) diverge from the arena's (4)


def AD(rid, n, gscale=3.0, norm=True, gates=None, nan_step=None, own_counts=True, **hyper):
    return pytest.param(dict(n=n, gscale=gscale, norm=norm, gates=gates, nan_step=nan_step, own_counts=own_counts, hyper=dict(HYPER, **hyper)), id=rid)


ADAM_ROWS = [
    AD('adam n1 clip active', 1),
    AD('adam n257 clip active', 257),
    AD('adam n10007 clip active', 10007),
    AD('adam n10007 grad_scale 1/128 norm below max_norm', 10007, gscale=128 * 0.005, grad_scale=1.0 / 128),
    AD('adam n257 grad_scale 1/128 clip active', 257, gscale=128 * 3.0, grad_scale=1.0 / 128),
    AD('adam n257 norm below max_norm', 257, gscale=0.01),
    AD('adam n10007 max_norm 0 no clip', 10007, max_norm=0.0),
    AD('adam n257 norm_finite NULL', 257, norm=False),
    AD('adam n257 wd 0 zero gradient p unchanged', 257, gscale=0.0, wd=0.0),
    AD('adam n10007 two ranges two flags', 10007, gates=dict(ranges=[(0, 1), (5000, 10007)], fidx=[0, 1], flags=PATTERN)),
    AD('adam n257 two ranges one flag', 257, gates=dict(ranges=[(3, 40), (100, 257)], fidx=[0, 0], flags=[[1], [0], [1], [1]])),
    AD('adam n1 one gated element', 1, gates=dict(ranges=[(0, 1)], fidx=[0], flags=[[0], [1], [0], [1]])),
    AD('adam n257 skipped step in the middle', 257, nan_step=1),
    # gates without gate_steps: the gated ranges are bias-corrected with the arena's count (include/mrdis.h), from step_state and from the host alike
    AD('adam n257 gates without gate_steps arena count', 257, gates=dict(ranges=[(0, 1), (100, 257)], fidx=[0, 1], flags=PATTERN), own_counts=False),
    AD('adam n10007 gates and a skipped step', 10007, gates=dict(ranges=[(0, 1), (5000, 10007)], fidx=[0, 1], flags=PATTERN), nan_step=1),
]


def adam_spec(row):
    n, gates = row['n'], row['gates']
    s = dict(p0=rnd((n,), 60), hyper=row['hyper'], norm=row['norm'], ranges=gates['ranges'] if gates else [], fidx=gates['fidx'] if gates else [],
             flags=gates['flags'] if gates else None, own_counts=row['own_counts'])
    grads = [rnd((n,), 61 + k, row['gscale']) for k in range(K_STEPS)]
    for k, g in enumerate(grads):          # a gated-off range holds no gradient: the arena's slots are zero
        if gates:
            for (lo, hi), f in zip(gates['ranges'], gates['fidx']):
                if not gates['flags'][k][f]:
                    g[lo:hi] = 0
    if row['nan_step'] is not None:
        grads[row['nan_step']][n // 2] = float('nan')
    s['grads'] = grads
    return s


def row_adam(row, impl, rec):
    s = adam_spec(row)
    ref = AC.adam_ref(s['p0'], s['grads'], s['flags'], s['ranges'], s['fidx'], clip=s['norm'], arena_count=not s['own_counts'], **s['hyper'])
    o = impl.adam(s)
    for name in ('p', 'm', 'v', 'vmax'):
        rec(name, ('adam', name), o[name], *ref[name])
    assert (o['applied'], o['skipped']) == (ref['applied'], ref['skipped']), ('step_state', o['applied'], o['skipped'], ref['applied'], ref['skipped'])
    if s['own_counts']:
        assert list(o['gate_steps']) == list(ref['gate_steps']), ('gate_steps', o['gate_steps'], ref['gate_steps'])
    if row['nan_step'] is not None and impl.gpu:
        assert len(o['skip_snaps']) == 1
    for before, after in o['skip_snaps']:          # a skipped step leaves p, m, v, vmax and gate_steps unchanged in their bits
        for a, b, name in zip(before, after, ('p', 'm', 'v', 'vmax', 'gate_steps')):
            bits_eq(b, a, f'{name} over a skipped step')
    if row['hyper']['wd'] == 0.0 and row['gscale'] == 0.0:
        bits_eq(o['p'], s['p0'], 'p under a zero gradient without weight decay')
    if not s['fidx'] or not s['own_counts']:          # the host step count must give the bits of the device counter (gate_steps needs step_state: the per-gate rows have no host form)
        h = impl.adam(s, host_step=True)
        for name in ('p', 'm', 'v', 'vmax'):
            bits_eq(h[name], o[name], f'{name}: host step count against step_state')


# ---------------------------------------------------------------- softmax with the dropped mask logit
SOFTMAX_ROWS = [pytest.param(dict(C=Cc, P=P, mask=mk), id=f"softmax C{Cc} P{P} {'mask' if mk else 'NULL'}")
                for Cc, P, mk in [(1, 1, True), (1, 257, False), (4, 257, True), (4, 1, False), (7, 257, True), (7, 257, False), (SM_MAXC, 257, True), (SM_MAXC, 1, False)]]


def row_softmax(row, impl, rec):
    Cc, P = row['C'], row['P']
    s = rnd((P, Cc), 70, 30.0).clamp(-80, 80)
    s[0, 0] = 80.0; s[-1, -1] = -80.0
    if P > 2:
        s[1] = -80.0; s[2] = 80.0
    mask = (torch.arange(P) % 3 != 0).float() if row['mask'] else None
    dout = rnd((P, Cc), 71)
    ref, A, extra = AC.softmax_md_ref(s, mask, 100.0)
    for pad in (0, PAD):
        tag = ' slice' if pad else ' dense'
        out = impl.softmax_fwd(s, mask, 100.0, pad)
        rec('out' + tag, ('softmax', 'out'), out, ref, A, extra=extra)
        ds = impl.softmax_bwd(dout, out, pad)
        rec('ds' + tag, ('softmax', 'ds'), ds, *AC.softmax_md_bwd_ref(dout, out), extra=extra)          # from the STORED output


# ---------------------------------------------------------------- reconstruction error
RECON_ROWS = [pytest.param(dict(N=N, HW=HW, C=Cc, p=p), id=f'recon p{p} N{N} HWC {HW}x{Cc}')
              for p in (1, 2) for N, HW, Cc in [(3, 120, 7), (1, 241, 17), (2, 647, 19), (64, 87383, 3), (4097, 1, 5)]]
assert 647 * 19 == 3 * 4096 + 5 and 87383 * 3 == 64 * 4096 + 5 and 241 * 17 == 4097


@functools.lru_cache(maxsize=2)
def recon_case(N, HW, Cc):
    gt, x = rnd((N, HW, Cc), 80), rnd((N, HW, Cc), 81)
    x.view(-1)[::7] = gt.view(-1)[::7]          # gt == x exactly: gradient 0 for p = 1
    return gt, x, rnd((N,), 82)


def row_recon(row, impl, rec):
    N, HW, Cc, p = (row[k] for k in ('N', 'HW', 'C', 'p'))
    gt, x, w = recon_case(N, HW, Cc)
    e, dx = AC.recon_err_ref(gt, x, p), AC.recon_err_bwd_ref(gt, x, w, p)
    for pad in (0, 1):
        tag = ' slice' if pad else ' dense'
        rec('err' + tag, ('recon', 'err'), impl.recon_fwd(gt, x, p, pad), *e)
        got = impl.recon_bwd(gt, x, w, p, pad)
        rec('dx' + tag, ('recon', 'dx'), got, *dx)
        if p == 1:
            assert not bool(got.reshape(-1)[::7].any()), 'gt == x must give gradient exactly 0'


# ---------------------------------------------------------------- max-pool (exact)
POOL_ROWS = [pytest.param(dict(N=N, C=Cc, H=H, W=W, k=k), id=f'maxpool k{k} {H}x{W} C{Cc}')
             for N, Cc, H, W, k in [(2, 3, 5, 7, 1), (2, 4, 9, 11, 2), (1, 5, 35, 50, 16), (2, 4, 16, 16, 16), (3, 2, 3, 3, 3), (1, 300, 7, 9, 2)]]


def row_maxpool(row, impl, rec):
    N, Cc, H, W, k = (row[n] for n in ('N', 'C', 'H', 'W', 'k'))
    x = rnd((N, Cc, H, W), 90)
    if k > 1:
        x[0, 0, 0, 1] = x[0, 0, 0, 0] = 9.0          # a tie: the first in scan order wins
        x[0, 0, k - 1, k - 1] = 9.0
        x[-1, -1, 0:k, 0:k] = float('-inf')          # a window of all -inf
        if H >= 2 * k:
            x[0, -1, k + 1, 0] = float('nan')        # a NaN in a window
        if W >= 2 * k:
            x[-1, 0, 0, k:2 * k] = 4.0               # a whole row of equal maxima
    y, arg = AC.maxpool_ref(x, k)
    for pad in (0, PAD):
        gy, garg = impl.maxpool_fwd(x, k, pad)
        bits_eq(gy, y, 'maxpool values'); int_eq(garg, arg, 'maxpool argmax')
        dy = rnd(tuple(y.shape), 91)
        dx = impl.maxpool_bwd(dy, garg, (N, Cc, H, W), k, pad)
        bits_eq(dx, AC.maxpool_bwd_ref(dy, arg, (N, Cc, H, W)), 'maxpool dx')
        Hk, Wk = H // k * k, W // k * k
        assert not bool(dx[:, :, Hk:].any()) and not bool(dx[:, :, :, Wk:].any()), 'the floor remainder gets gradient exactly 0'


# ---------------------------------------------------------------- cast_view (exact)
CAST_ROWS = [pytest.param(dict(src=a, dst=b, Cs=cs, Cd=cd), id=f"cast {'bf16' if a is B16 else 'f32'}->{'bf16' if b is B16 else 'f32'} C{cs}->{cd}")
             for a in (F32, B16) for b in (F32, B16) for cs, cd in [(7, 16), (4, 16), (16, 7), (16, 4), (5, 5), (8, 8)]]


def cast_values(shape, dtype):
    """random values with, in front, exact bf16 rounding ties in both directions (kept mantissa even: down; odd: up), +-0, +-inf, +-FLT_MAX"""
    x = rnd(shape, 95)
    i = x.view(torch.int32)
    flat = i.view(-1)
    n = flat.numel() // 3
    flat[:n] = (flat[:n] & -65536) | 0x8000          # ties: the bits below bf16 are exactly one half
    x.view(-1)[n:n + 6] = torch.tensor([0.0, -0.0, float('inf'), float('-inf'), 3.4028234663852886e38, -3.4028234663852886e38])
    return x.to(dtype)          # (a bf16 source holds the rounded values: widening them is exact)


def row_cast(row, impl, rec):
    Cs, Cd = row['Cs'], row['Cd']
    x = cast_values((2, Cs, 5, 7), row['src'])
    ref = AC.cast_view_ref(x, row['dst'], Cd)
    if row['src'] is F32 and row['dst'] is B16:          # the reference itself rounds to nearest even: ties go to the even neighbour, not toward zero
        t = x[:, :min(Cs, Cd)]
        trunc = (t.view(torch.int32) & -65536).view(F32)
        assert bool((ref[:, :min(Cs, Cd)].float() != trunc)[torch.isfinite(t)].any())
    for mode in ('dense', 'slice', 'off1'):
        v1 = bool(Cs % 4 or Cd % 4 or mode == 'off1')
        y = impl.cast_view(x, row['dst'], Cd, mode, v1)
        assert y.dtype is row['dst']
        bits_eq(y, ref, f'cast_view {mode}')


# ---------------------------------------------------------------- slice_gather (exact)
def SG(rid, M, block, H, W, B, ld_extra=0, px=True):
    return pytest.param(dict(M=M, block=block, H=H, W=W, B=B, ld_extra=ld_extra, px=px), id=rid)


GATHER_ROWS = [
    SG('gather px M4 block3 15x17', 4, 3, 15, 17, 3), SG('gather px M4 block0 15x17', 4, 0, 15, 17, 3), SG('gather px M8 block1 1x1', 8, 1, 1, 1, 3),
    SG('gather px M4 block3 513x513 over the block cap', 4, 3, 513, 513, 1),
    SG('gather contrast M3 block3 15x17', 3, 3, 15, 17, 3, px=False), SG('gather contrast M4 block4 1x1', 4, 4, 1, 1, 3, px=False),
    SG('gather contrast M4 block3 ld not 4n', 4, 3, 15, 17, 3, ld_extra=1, px=False), SG('gather contrast M3 block3 513x513', 3, 3, 513, 513, 1, px=False),
]


def row_gather(row, impl, rec):
    """every row twice: with the row's own pitch (dense unless it says otherwise) and into a wider NaN-prefilled `inputs` -- 4 more columns for the
    per-pixel rows (they stay on that kernel), an odd 3 for the per-contrast rows -- whose extra columns keep their NaN bits (HipImpl.slice_gather)"""
    M, block, H, W, B = (row[k] for k in ('M', 'block', 'H', 'W', 'B'))
    Cc = M * (2 * block + 1)
    pitches = (row['ld_extra'], 4 if row['px'] else 3)
    for ldx in pitches:
        assert row['px'] == (Cc % 4 == 0 and Cc <= 32 and (Cc + ldx) % 4 == 0), 'the row states the wrong kernel'
    D = 2 * block + 4
    vols = [[rnd((D, H, W), 1000 + 10 * b + m) for m in range(M)] for b in range(B)]
    for b in range(B):
        vols[b][0][:, 0, 0] = -0.0          # -0.0 in the first channel counts as zero
        vols[b][0][:, H // 2, W // 2] = 0.0
    slice_idx = [block, D - 1 - block, block + 1][:B]          # both clamped ends
    drop = [-1, 1 % M, 0][:B]
    if B > 1:
        vols[1][M - 1] = None               # a missing contrast
        vols[1][0] = vols[0][0]             # two samples sharing one volume
    if B > 2:
        vols[2][0] = None                   # contrast 0 missing and dropped: mask_img all ones
    want = AC.slice_gather_ref(vols, slice_idx, drop, H, W, D, block)
    if B > 2:
        assert bool((want[2][2] == 1).all())
    for ldx in pitches:
        got = impl.slice_gather(vols, slice_idx, drop, H, W, D, block, ldx)
        for g, w, name in zip(got, want, ('inputs', 'mask', 'mask_img')):
            bits_eq(g, w, f'slice_gather {name} (ld = C + {ldx})')


def row_limits(row, impl, rec):
    for fn in ('mix_limits', 'adam_limits', 'softmax_limits', 'slice_gather_limits'):
        r = getattr(impl, fn)()
        if r is not None:
            assert r[0] == r[1], (fn, r)


OPS = dict(mix=(row_mix, MIX_ROWS), mix1=(row_mix1, MIX1_ROWS), mix_jobs=(row_mix_jobs, [pytest.param({}, id='mix job table T 1 9 16 25')]),
           sumsq=(row_sumsq, SUMSQ_ROWS), adam=(row_adam, ADAM_ROWS), softmax=(row_softmax, SOFTMAX_ROWS), recon=(row_recon, RECON_ROWS),
           maxpool=(row_maxpool, POOL_ROWS), cast=(row_cast, CAST_ROWS), gather=(row_gather, GATHER_ROWS),
           limits=(row_limits, [pytest.param({}, id='refused geometries and short workspaces')]))
ALL_ROWS = [pytest.param(op, p.values[0], id=p.id) for op, (_, rows) in OPS.items() for p in rows]


def run_row(op, row, impl, rid, enforce):
    rec = Rec(rid, enforce)
    OPS[op][0](row, impl, rec)
    return rec.items


@pytest.mark.parametrize('op,row', ALL_ROWS)
def test_aux_path(mrdis, request, op, row):
    rid = request.node.callspec.id
    items = run_row(op, row, HipImpl(mrdis), rid, enforce=not MEASURING)
    if MEASURING:
        yard = {name: r for name, _, r in run_row(op, row, TorchImpl(), rid, False)}
        for name, key, r in items:
            dump_measured('aux_path_margins.jsonl', dict(row=rid, out=name, key=list(key), kernel=r, yardstick=yard.get(name), kappa=AC.KAPPA.get(key)))
        for name, key, r in items:
            assert key in AC.KAPPA and r <= AC.KAPPA[key], f'{rid}: {name} needs kappa {r:.2f}, committed {AC.KAPPA.get(key)}'
