"""The `others` variants of the reference (config.yaml:67-70: mod_enc_s, ana_dec_act softplus / plain softmax) on the MI355X:
the new kernels (csrc/mrdis_encs.hip) element-wise against float64, one training step per variant against vectors from the real
reference (tools/gen_golden_variants.py), graph replay, the live gradient path through the second pass's anatomy maps, and the
entry point."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

import conv_check as CC
from fixtures import make_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device('cuda:0')
PAD_C = 3

ENCS = {'mod_enc_s': True, 'ana_dec_act': 'softmax', 'old': False}
SOFTPLUS = {'mod_enc_s': False, 'ana_dec_act': 'softplus', 'old': False}
ENCS_SOFTPLUS = {'mod_enc_s': True, 'ana_dec_act': 'softplus', 'old': False}


@pytest.fixture(scope='module')
def mrdis():
    import mrdis as m
    assert torch.cuda.is_available()
    m.hip.load()
    return m


def cl(x):
    return x.to(DEV).contiguous(memory_format=torch.channels_last)


def rnd(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def in_slice(t, seed):
    """t (N, C, H, W) as a channel slice of a wider NHWC device buffer"""
    N, C, H, W = t.shape
    wide = torch.cat([rnd((N, PAD_C, H, W), seed), t, rnd((N, PAD_C, H, W), seed + 1)], 1)
    return cl(wide)[:, PAD_C:PAD_C + C]


def out_slice(N, C, H, W):
    buf = torch.empty((N, C + 2 * PAD_C, H, W), device=DEV, memory_format=torch.channels_last).fill_(float('nan'))
    return buf, buf[:, PAD_C:PAD_C + C]


def untouched(buf, C, what):
    nan = torch.full((1,), float('nan')).view(torch.int32).item()
    for side in (buf[:, :PAD_C], buf[:, PAD_C + C:]):
        assert bool((side.contiguous().view(torch.int32) == nan).all()), f'{what}: a store landed outside the output channel slice'


# ------------------------------------------------------------------------------------------------ two-source convolution vs float64
# kappa: fp32 FMA chains of T * (Cx + Cs) <= 99 terms (forward, data gradient: one chain per element) and of 64 pixels per tile, then
# the tiles of a workgroup and the ordered slab sum (weight gradient).  Both are about 4x the worst ratio measured on the MI355X.
KAPPA_2SRC = {'fwd': 8, 'dx': 8, 'ds': 8, 'dw': 16, 'db': 16}
GEOMS = [  # (N, Cx, Cs, H, W, Co, k, stride, pad)
    (1, 7, 4, 13, 11, 16, 3, 2, 1),          # B = 1, odd sizes
    (2, 7, 8, 17, 23, 16, 3, 2, 1),          # Cin_s = 8
    (3, 7, 4, 66, 70, 16, 3, 2, 1),          # Wo = 35: a partial weight-gradient tile
    (2, 7, 4, 130, 131, 12, 3, 2, 1),        # Co = 12 < 16, Wo = 66: two tiles per row, the second nearly empty
    (1, 7, 4, 9, 10, 16, 3, 1, 1),           # stride 1
    (2, 7, 20, 15, 19, 16, 3, 2, 1),         # Cx + Cs = 27 > 16: the 32-channel data-gradient form, 244 weight-gradient jobs
    (2, 9, 23, 11, 12, 16, 3, 1, 0),         # Cx + Cs = 32 (the limit), pad 0, one weight-gradient job copy per workgroup
    (3, 5, 3, 14, 17, 8, 2, 2, 0),           # 2x2 filter, pad 0, Co = 8
]


@pytest.mark.parametrize('geom', GEOMS, ids=lambda g: 'N{}_Cx{}_Cs{}_{}x{}_Co{}_k{}s{}p{}'.format(*g))
def test_two_source_conv_vs_float64(mrdis, geom):
    hip = mrdis.hip
    N, Cx, Cs, H, W, Co, k, st, pad = geom
    Ho, Wo = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
    Ci = Cx + Cs
    x, s = rnd((N, Cx, H, W), 1), rnd((N, Cs, H, W), 2).softmax(1)
    w, b = rnd((Co, Ci, k, k), 3, (Ci * k * k) ** -0.5), rnd((Co,), 4, 0.1)
    dy = rnd((N, Co, Ho, Wo), 5)
    w_tck = w.permute(2, 3, 1, 0).reshape(-1, Ci, Co).contiguous().to(DEV)
    w_tkc = w.permute(2, 3, 0, 1).reshape(-1, Co, Ci).contiguous().to(DEV)
    xs = torch.cat([x, s], 1)
    xg, sg = in_slice(x, 10), in_slice(s, 20)
    dyg = in_slice(dy, 30)
    hip.launch_counts(reset=True)
    for lrelu in (False, True):
        buf, y = out_slice(N, Co, Ho, Wo)
        hip.conv2d_2src_fwd(xg, sg, w_tck, b.to(DEV), k, k, st, pad, lrelu, out=y)
        ref, A = CC.fwd_ref(xs, w, b, st, pad, lrelu)
        CC.check(y, ref, A, KAPPA_2SRC['fwd'], what=f'fwd lrelu={lrelu}')
        untouched(buf, Co, 'fwd')
    ref, A = CC.dgrad_ref(dy, w, (H, W), st, pad)
    bx, dx = out_slice(N, Cx, H, W)
    bs, ds = out_slice(N, Cs, H, W)
    got_dx, got_ds = hip.conv2d_2src_bwd_data(dyg, w_tkc, Cx, Cs, (H, W), k, k, st, pad, dx_out=dx, ds_out=ds)
    CC.check(got_dx, ref[:, :Cx], A[:, :Cx], KAPPA_2SRC['dx'], what='dx')
    CC.check(got_ds, ref[:, Cx:], A[:, Cx:], KAPPA_2SRC['ds'], what='ds')
    untouched(bx, Cx, 'dx'); untouched(bs, Cs, 'ds')
    bs2, ds2 = out_slice(N, Cs, H, W)
    none_dx, _ = hip.conv2d_2src_bwd_data(dyg, w_tkc, Cx, Cs, (H, W), k, k, st, pad, need_dx=False, ds_out=ds2)
    assert none_dx is None and torch.equal(ds2, ds)
    dw_ref, A_dw, db_ref, A_db = CC.wgrad_ref(xs, dy, k, k, st, pad)
    wide = torch.full((k * k * Ci * Co + 64,), float('nan'), device=DEV)
    dw, db = hip.conv2d_2src_bwd_weight(xg, sg, dyg, k, k, st, pad, dw_out=wide[:k * k * Ci * Co].view(k * k, Ci, Co))
    CC.check(dw.view(k, k, Ci, Co).permute(3, 2, 0, 1), dw_ref, A_dw, KAPPA_2SRC['dw'], what='dw')
    CC.check(db, db_ref, A_db, KAPPA_2SRC['db'], what='db')
    assert bool(torch.isnan(wide[k * k * Ci * Co:]).all()), 'dw: a store landed past the filter'
    sink = torch.full((Co,), 0.5, device=DEV)
    dw2, none_db = hip.conv2d_2src_bwd_weight(xg, sg, dyg, k, k, st, pad, bias_sink=sink)
    assert none_db is None and torch.equal(dw2, dw)
    CC.check(sink - 0.5, db_ref, A_db + 1.0, KAPPA_2SRC['db'], what='bias sink')
    assert hip.launch_counts()['conv2src'] == 2 + 2 + 2


# ------------------------------------------------------------------------------------------------ anatomy activations vs float64
def _act_input(N=2, C=4, H=9, W=13):
    x = rnd((N, C, H, W), 7, 6.0)
    special = torch.tensor([-100., -30., -20.5, -1e-3, 0., 1e-3, 19.99, 20., 20.0001, 20.5, 25., 100.])
    x.view(-1)[:special.numel()] = special
    x.view(-1)[-special.numel():] = special.flip(0)
    return x


def test_softplus_vs_float64_and_torch_threshold(mrdis):
    hip = mrdis.hip
    x = _act_input()
    N, C, H, W = x.shape
    xg, dyg = in_slice(x, 40), in_slice(rnd(x.shape, 8), 50)
    dy = rnd(x.shape, 8)
    hip.launch_counts(reset=True)
    buf, y = out_slice(N, C, H, W)
    hip.softplus_fwd(xg, out=y)
    ref = F.softplus(x.double())                                   # beta 1, threshold 20
    CC.check(y, ref, ref.abs(), 8, what='softplus fwd')
    untouched(buf, C, 'softplus fwd')
    big = x > 20
    assert torch.equal(y.cpu()[big], x[big])                       # the threshold rule: the input itself, bit for bit
    buf, dx = out_slice(N, C, H, W)
    hip.softplus_bwd(dyg, xg, out=dx)
    ref = torch.where(x.double() > 20, dy.double(), dy.double() * torch.sigmoid(x.double()))
    CC.check(dx, ref, ref.abs(), 8, what='softplus bwd')
    untouched(buf, C, 'softplus bwd')
    assert torch.equal(dx.cpu()[big], dy[big])
    assert hip.launch_counts()['ana_act'] == 2


def test_plain_softmax_vs_float64(mrdis):
    hip = mrdis.hip
    s = _act_input()
    N, C, H, W = s.shape
    dout = rnd(s.shape, 9)
    sg, dg = in_slice(s, 60), in_slice(dout, 70)
    hip.launch_counts(reset=True)
    buf, y = out_slice(N, C, H, W)
    hip.softmax_fwd(sg, out=y)
    ref = torch.softmax(s.double(), 1)
    # exp's condition number is its argument: an output e^(s - max) / den carries the rounding of s - max times |s - max|
    A = ref * (2.0 + (s.double() - s.double().amax(1, keepdim=True)).abs())
    CC.check(y, ref, A, 4 * C, what='softmax fwd')
    untouched(buf, C, 'softmax fwd')
    o = y.detach().double().cpu()                                  # the backward reads the forward's stored output
    buf, ds = out_slice(N, C, H, W)
    hip.softmax_bwd(dg, y, out=ds)
    dot = (o * dout.double()).sum(1, keepdim=True)
    ref = o * (dout.double() - dot)
    A = o * (dout.double().abs() + (o * dout.double()).abs().sum(1, keepdim=True))
    CC.check(ds, ref, A, 4 * C, what='softmax bwd')
    untouched(buf, C, 'softmax bwd')
    assert hip.launch_counts()['ana_act'] == 2


# ------------------------------------------------------------------------------------------------ one step vs the real reference
def _cfg(mrdis, M, H, W, B, others, **kw):
    cfg = dict(mrdis.DEFAULT_CONFIG)
    cfg.update(contrast_list=[f'm{i}' for i in range(M)], input_height=H, input_width=W, batch_size=max(B, 16), others=dict(others), **kw)
    return mrdis.derive_config(cfg, DEV)


class _ConcatSpy:
    """records the input-channel counts of every filter ops.conv2d / torch.ops.mrdis.cond_conv2d receive: the concatenated first layer
    would show up as one of Cx + Cs = 11 channels"""

    def __init__(self, mrdis, monkeypatch):
        self.ci = []
        ops = mrdis.ops
        conv2d = ops.conv2d

        def spy(x, w_tck, *a, **k):
            self.ci.append(w_tck.shape[1])
            return conv2d(x, w_tck, *a, **k)
        monkeypatch.setattr(ops, 'conv2d', spy)


VARIANT_GOLDENS = [('b2m2_encs', ENCS), ('b2m2_softplus', SOFTPLUS), ('b2m4_encs_softplus_drop', ENCS_SOFTPLUS)]


@pytest.mark.parametrize('tag,others', VARIANT_GOLDENS, ids=[t for t, _ in VARIANT_GOLDENS])
def test_variant_train_step_golden(mrdis, golden_dir, monkeypatch, tag, others):
    meta = json.load(open(os.path.join(golden_dir, f'step_{tag}.json')))
    arrs = np.load(os.path.join(golden_dir, f'step_{tag}.npz'))
    B, M = meta['B'], meta['M']
    cfg = _cfg(mrdis, M, 160, 192, B, others)
    torch.manual_seed(10); np.random.seed(10)
    model = mrdis.build_model(cfg).train()
    reads_s = others['mod_enc_s']
    assert model.modality_encoder_reads_s() == reads_s
    for k, v in meta['wsum_before'].items():
        got = float(model.state_dict()[k].double().sum())
        assert abs(got - v) <= 1e-6 * max(1.0, abs(v)), ('init', k)
    inputs, mask, mask_img = make_inputs(B, M, 160, 192, seed=10, drop=meta['drop'])
    step = mrdis.TrainStep(model, cfg)
    spy = _ConcatSpy(mrdis, monkeypatch)
    mrdis.hip.launch_counts(reset=True)
    torch.manual_seed(11); np.random.seed(11)
    names = {id(p): n for n, p in model.named_parameters()}
    with mrdis.ops.mix_cache():
        loss, parts, aux = mrdis.forward_losses(model, cfg, cl(inputs), mask.to(DEV), mask_img.to(DEV), mask)
        loss.backward()
    counts = mrdis.hip.launch_counts()
    assert counts['ana_act'] >= (2 if reads_s else 1) * M, counts                   # activation forward: both encoder passes when the maps are read
    assert (counts['conv2src'] >= 2 * M) if reads_s else counts['conv2src'] == 0, counts             # (forward: both passes, every modality)
    assert 7 + 4 not in spy.ci, 'the concatenated first layer ran'
    assert abs(float(loss) - meta['loss']) <= 1e-3 * abs(meta['loss']), (float(loss), meta['loss'])
    for k, v in meta['parts'].items():
        assert abs(float(parts[k]) - v) <= 1e-3 * abs(v) + 1e-6, (k, float(parts[k]), v)
    close = _close
    close(torch.stack(aux['mu_list']), arrs['mu'], 'mu'); close(torch.stack(aux['zi_list']), arrs['z'], 'z')
    close(F.avg_pool2d(aux['si_list'][0], 8), arrs['s0_pool8'], 's0')
    close(F.avg_pool2d(aux['xi_fake_list'][0], 8), arrs['xf0_pool8'], 'xf0')
    close(F.avg_pool2d(aux['xi_fake_mix_list'][0], 8), arrs['xmix0_pool8'], 'xmix0')
    gn = {names[id(p)]: float(p.grad.double().norm()) for p in model.parameters() if p.grad is not None}
    hot = {k: v for k, v in meta['grad_norms'].items() if not k.startswith('output_decoder')}
    assert set(hot) == set(gn)
    if reads_s:
        # the two-source layer's filter gradient on its own scale (the bound below is floored by the step's total norm, which dwarfs it)
        k1 = 'modality_encoder_list.0.conv1.weight'
        print(f'{tag}: conv1 weight gradient norm {gn[k1]:.6e} vs reference {hot[k1]:.6e} (rel {abs(gn[k1] - hot[k1]) / hot[k1]:.2e})')
        assert abs(gn[k1] - hot[k1]) <= 1e-4 * hot[k1], (gn[k1], hot[k1])          # measured 1.3e-7
    total = float(np.sqrt(sum(v * v for v in gn.values())))
    ref_total = float(np.sqrt(sum(v * v for v in hot.values())))
    assert abs(total - ref_total) <= 1e-3 * ref_total, (total, ref_total)
    worst = max((abs(gn[k] - v) / (v + 4e-3 * ref_total), k) for k, v in hot.items())
    print(f'{tag}: worst per-tensor gradient-norm deviation {worst[0]:.2e} ({worst[1]})')
    for k, v in hot.items():
        assert abs(gn[k] - v) <= 1e-3 * (v + 4e-3 * ref_total), (k, gn[k], v)
    step.optimizer.step(fused_clip=True)
    for k, v in meta['wsum_after'].items():
        if meta['grad_norms'].get(k, 1.0) < 1e-5 * meta['grad_norm']:
            continue
        t = model.state_dict()[k]
        got = float(t.double().sum())
        flips = 2 * cfg['lr'] * np.ceil(1e-3 * t.numel())
        assert abs(got - v) <= 2e-4 * max(1.0, abs(v)) + flips, ('after step', k, got, v)


def _close(got, want, what, rtol=1e-3):
    got = got.detach().float().cpu()
    want = torch.as_tensor(want).float()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), what
    err = (got - want).abs().max().item()
    assert err <= rtol * float(want.abs().max()) + 1e-7, (what, err, float(want.abs().max()))


# ------------------------------------------------------------------------------------------------ graph replay, bf16m, dead maps
def _batches(mrdis, n, B, M, H, W):
    out = []
    for seed in range(40, 400):
        if len(out) == n:
            break
        x, mask, mask_img = mrdis.synthetic_batch(B, M, H, W, seed=seed, drop=True)
        if mrdis.regular_mask(mask):
            out.append((cl(x), mask, mask_img.to(DEV)))
    assert len(out) == n
    return out


def _run(mrdis, graph, steps, others, B=8, M=4, H=64, W=96, dtype='f32'):
    cfg = _cfg(mrdis, M, H, W, 16, others, lambda_adv_s=1.0, compute_dtype=dtype)
    torch.manual_seed(10); np.random.seed(10)
    model = mrdis.build_model(cfg).train()
    step = mrdis.TrainStep(model, cfg)
    if graph:
        step = mrdis.GraphedTrainStep(step)
    data = _batches(mrdis, steps, B, M, H, W)
    torch.manual_seed(100); np.random.seed(100)
    losses = []
    try:
        for x, mask, mask_img in data:
            loss, parts, _ = step(x, mask.to(DEV), mask_img, mask)
            losses.append({k: float(v) for k, v in parts.items()})
        torch.cuda.synchronize()
    finally:
        mrdis.ops.set_compute_dtype('f32')
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu()
    bufs = torch.cat([b.detach().float().reshape(-1) for b in model.buffers()]).cpu()
    return flat, bufs, losses, step


@pytest.mark.timeout(900)
def test_graph_replay_is_bit_identical_for_mod_enc_s_softplus(mrdis):
    """GraphedTrainStep against the eager step over 8 steps whose drop-off masks change every iteration (mod_enc_s + softplus)"""
    ref_w, ref_b, ref_l, _ = _run(mrdis, False, 8, ENCS_SOFTPLUS)
    got_w, got_b, got_l, step = _run(mrdis, True, 8, ENCS_SOFTPLUS)
    assert step.stats['replays'] > 0, step.stats
    assert got_l == ref_l
    assert torch.equal(ref_w, got_w), float((ref_w - got_w).abs().max())
    assert torch.equal(ref_b, got_b)


@pytest.mark.parametrize('others', [ENCS, SOFTPLUS], ids=['encs', 'softplus'])
def test_bf16m_compute_runs_the_variants(mrdis, others):
    """compute_dtype 'bf16m' (bf16 MFMA operands, fp32 activations): two steps, finite and close to the f32 step"""
    w32, _, l32, _ = _run(mrdis, False, 2, others)
    w16, _, l16, _ = _run(mrdis, False, 2, others, dtype='bf16m')
    assert torch.isfinite(w16).all() and all(np.isfinite(v) for l in l16 for v in l.values())
    for k, v in l32[0].items():                                    # the first step (later ones drift: the discriminator loss amplifies it)
        assert abs(v - l16[0][k]) <= 2e-2 * abs(v) + 1e-4, (k, v, l16[0][k])


def test_bf16_storage_names_the_variant(mrdis):
    cfg = _cfg(mrdis, 2, 64, 64, 4, ENCS, compute_dtype='bf16')
    try:
        with pytest.raises(NotImplementedError, match='mod_enc_s'):
            mrdis.build_model(cfg)
    finally:
        mrdis.ops.set_compute_dtype('f32')


def test_second_pass_maps_are_live_under_mod_enc_s(mrdis, monkeypatch):
    """main_missing.py:228-231 under mod_enc_s: the second encoder pass computes its anatomy maps (the modality encoder reads them), and the
    gradient through them reaches the anatomy network -- cutting it (the maps of that pass detached) changes the anatomy network's gradients."""
    B, M, H, W = 2, 2, 64, 96
    inputs, mask, mask_img = make_inputs(B, M, H, W, seed=10)
    res = {}
    for cut in (False, True):
        cfg = _cfg(mrdis, M, H, W, B, ENCS_SOFTPLUS)
        torch.manual_seed(10); np.random.seed(10)
        model = mrdis.build_model(cfg).train()
        orig = model.compute_anatomy_encoding
        calls = []

        def spy(inputs_list, mask_img_, need_maps=True):
            out = orig(inputs_list, mask_img_, need_maps=need_maps)
            calls.append(need_maps and all(s is not None for s in out))
            if cut and len(calls) == 2:
                out = [s.detach() for s in out]
            return out
        monkeypatch.setattr(model, 'compute_anatomy_encoding', spy)
        step = mrdis.TrainStep(model, cfg)
        torch.manual_seed(11); np.random.seed(11)
        with mrdis.ops.mix_cache():
            loss, parts, _ = mrdis.forward_losses(model, cfg, cl(inputs), mask.to(DEV), mask_img.to(DEV), mask)
            loss.backward()
        assert calls == [True, True], calls                       # both passes computed their maps
        res[cut] = {n: p.grad.detach().clone() for n, p in model.named_parameters()
                    if p.grad is not None and n.startswith(('anatomy_encoder_enc_list.', 'anatomy_encoder_dec.'))}
        del step
    assert set(res[False]) == set(res[True]) and res[False]
    diff = [n for n in res[False] if not torch.equal(res[False][n], res[True][n])]
    assert len(diff) > len(res[False]) // 2, (len(diff), len(res[False]))


# ------------------------------------------------------------------------------------------------ entry point
@pytest.mark.timeout(900)
def test_entry_point_trains_and_evaluates_mod_enc_s_softplus(tmp_path):
    """main_missing.py with others = {'mod_enc_s': True, 'ana_dec_act': 'softplus', 'old': False} in config.yaml on synthetic data: one epoch of
    two training steps with its validation pass, then the test phase from the saved checkpoint, each in a fresh process.  (The synthetic test
    split holds one subject, so the nearest-neighbour search would have no other subject to search: the test phase runs with the slices' own codes.)"""
    base = dict(contrast_list=['T1', 'T2'], input_height=64, input_width=64, batch_size=20, epochs=1, gpu='0', data_source='synthetic',
                ckpt_root=str(tmp_path / 'ckpt'), others=dict(ENCS_SOFTPLUS), lambda_adv_s=1.0)
    (tmp_path / 'config.yaml').write_text(yaml.dump(base))
    script = os.path.join(ROOT, 'main_missing.py')
    r = subprocess.run([sys.executable, script, str(tmp_path / 'config.yaml')], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ck = os.path.join(str(tmp_path / 'ckpt'))
    found = [os.path.join(d, f) for d, _, fs in os.walk(ck) for f in fs]
    stat = [f for f in found if f.endswith('stat.csv')]
    assert stat and any(f.endswith('model_best.pth.tar') for f in found), found
    rows = open(stat[0]).read().strip().split('\n')
    assert len(rows) == 3 and rows[2].split(',')[1] == 'val', rows
    sd = torch.load([f for f in found if f.endswith('model_best.pth.tar')][0], map_location='cpu', weights_only=False)['model']
    assert tuple(sd['modality_encoder_list.0.conv1.weight'].shape) == (3, 16, 11, 3, 3)
    label = os.path.basename(os.path.dirname(stat[0]))                  # the training run's directory (named by its start time)
    (tmp_path / 'test.yaml').write_text(yaml.dump(dict(base, phase='test', ckpt_timelabel=label)))
    r = subprocess.run([sys.executable, script, str(tmp_path / 'test.yaml')], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'psnr' in r.stdout, r.stdout[-2000:]


@pytest.mark.timeout(900)
def test_nearest_neighbour_evaluation_under_mod_enc_s(mrdis, tmp_path, monkeypatch):
    """build_z_gallery and Run.evaluate(info='nearest_neighbour' | 'mean') on a mod_enc_s + softplus model (the modality encoder reads the
    anatomy maps): a synthetic test split of two subjects, the search kernel and the two-source layer both run, the usual stats come back"""
    store = mrdis.train.synthetic_store
    monkeypatch.setattr(mrdis.train, 'synthetic_store', lambda config, device: store(config, device, n_subj=10))      # a test split of two subjects
    base = dict(contrast_list=['T1', 'T2'], input_height=64, input_width=64, batch_size=4, epochs=1, gpu='0', data_source='synthetic',
                ckpt_root=str(tmp_path / 'ckpt'), ckpt_timelabel='t0', shuffle=False, others=dict(ENCS_SOFTPLUS))
    (tmp_path / 'train.yaml').write_text(yaml.dump(base))
    cfg = mrdis.train.setup_config(str(tmp_path / 'train.yaml'), device=DEV)
    run = mrdis.train.Run(cfg, log=lambda *a: None)
    assert run.model.modality_encoder_reads_s()
    run.train(max_iters_per_epoch=2)
    mrdis.hip.launch_counts(reset=True)
    gal = mrdis.build_z_gallery(run, run.loaders['test'])
    assert mrdis.hip.launch_counts()['conv2src'] > 0                 # the gallery's codes come from the encoder that reads s
    assert len(gal.subjects) >= 2 and torch.isfinite(gal.z).all()
    for info in ('nearest_neighbour', 'mean'):
        mrdis.hip.launch_counts(reset=True)
        stat = run.evaluate(phase='test', set_='test', info=info)
        c = mrdis.hip.launch_counts()
        assert c['conv2src'] > 0 and c['ana_act'] > 0
        if info == 'nearest_neighbour':
            assert c['zsearch'] >= 2
        assert {'rmse', 'psnr', 'ssim', 'recon_x_mix', 'all'} <= set(stat) and np.isfinite(stat['all'])
