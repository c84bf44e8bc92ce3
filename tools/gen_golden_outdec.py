"""Golden fixtures for the reference's output decoders other than 'U+SA' (target_model_name 'U', 'U+SA+CA', 'U+SSA+CA', model.py:261-299,
1002-1137, 1389-1433), the softplus target activation and the fuse methods (model.py:2951-2964, 3230-3258).  One training step of the real
reference model on the CPU per step fixture, recorded like oracle/gen_golden.py's recon_y fixture (loss parts, gradient norms of every
parameter and weight sums before and after Adam as name / value columns in the .npz, y0 / y1 pooled by 8), plus one checkpoint layout
of the output_decoder.* names and shapes for every decoder and fuse method.  Uses oracle/gen_golden.py's helpers as they are; writes new files under tests/golden/ only, the same
bytes on every run.

    python tools/gen_golden_outdec.py              # all fixtures (a few minutes of CPU)
    python tools/gen_golden_outdec.py ussaca_sp    # one of them (tags below)
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import gen_golden as G      # noqa: E402
from fixtures import make_inputs, make_seg_targets      # noqa: E402  (tests/ is on sys.path through gen_golden)
from fixtures_outdec import DECODERS, FUSE_METHODS, make_float_targets      # noqa: E402

SHIPPED_OTHERS = {'mod_enc_s': False, 'ana_dec_act': 'softmax', 'old': False, 'softmax_remove_mask': True}

# tag -> step arguments.  BraTS: segmentation loss, 4 output channels, activations 'no' (main_missing.py:80).  'sp': a non-BraTS dataset with
# norm_type 'mean', so both activations are softplus (main_missing.py:75-79) and recon_y is the p = 1 loss against float targets.
FIXTURES = {
    'u': dict(tag='b2m2_u', decoder='U', fuse='mean', brats=True),
    'uca': dict(tag='b2m2_uca', decoder='U+SA+CA', fuse='mean', brats=True),
    'ussaca': dict(tag='b2m2_ussaca', decoder='U+SSA+CA', fuse='mean', brats=True),
    'ussaca_sp': dict(tag='b2m2_ussaca_sp', decoder='U+SSA+CA', fuse='mean-max-min', brats=False),
    'layout': None,
}
B, M, H, W = 2, 2, 160, 192
TARGET_SEED = 13


def build_ref(ref, decoder, fuse, brats, out_num_ch):
    """gen_golden.build_ref_model with the decoder, fuse method and activations set (same arguments otherwise)"""
    act = 'no' if brats else 'softplus'
    return G.quiet(
        ref.MultimodalModel, input_size=(H, W), modality_num=M, in_num_ch=7, out_num_ch=out_num_ch,
        s_num_ch=4, z_size=16, is_cond=True, is_discrim_s=False, is_distri_z=False,
        s_compact_method='max', s_sim_method='cosine', z_sim_method='cosine', shared_ana_enc=True,
        shared_mod_enc=True, shared_inp_dec=False, device=torch.device('cpu'),
        input_output_act=act, target_output_act=act, target_model_name=decoder, fuse_method=fuse,
        others=dict(SHIPPED_OTHERS))


def gen_step(ref, tag, decoder, fuse, brats):
    """main_missing.py:175-251 for one batch with the shipped loss weights plus lambda_recon_y = 1 (gen_golden.gen_step's recon_y order)"""
    lam = dict(recon_x=1.0, recon_x_mix=2.0, latent_z=0.1, sim_s=10.0, sim_z=2.0, recon_y=1.0)
    out_num_ch = 4 if brats else 1
    torch.manual_seed(10); np.random.seed(10)                       # main_missing.py:18-21
    model = build_ref(ref, decoder, fuse, brats, out_num_ch)
    prefixes = G.HOT_PREFIXES + ('output_decoder.',)
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=2e-4, weight_decay=1e-5, amsgrad=True)
    inputs, mask, mask_img = make_inputs(B, M, H, W, seed=10, drop=False)
    targets = make_seg_targets(B, H, W, seed=TARGET_SEED) if brats else make_float_targets(B, H, W, seed=TARGET_SEED)
    torch.manual_seed(11); np.random.seed(11)
    w0 = {k: float(v.double().sum()) for k, v in model.state_dict().items() if k.startswith(prefixes) and v.dtype.is_floating_point}

    x_list = [inputs[:, i * 7:(i + 1) * 7] for i in range(M)]
    s_list = model.compute_anatomy_encoding(x_list, mask_img)
    z_list, mu_list, lv_list = model.compute_modality_encoding(x_list, s_list, phase='train')
    xf = model.reconstruct_input_si_zi(s_list, z_list)
    xmix = model.reconstruct_input_si_zj(s_list, z_list)
    parts = {}
    y_list = model.reconstruct_output_si(s_list)
    if brats:
        parts['recon_y'] = model.compute_segmentation_loss_y_list(targets, y_list, mask)
    else:
        parts['recon_y'] = model.compute_recon_loss_y_list(targets, y_list, mask, p=1)
    loss = lam['recon_y'] * parts['recon_y']
    parts['recon_x'] = model.compute_recon_loss_x_list(x_list, xf, mask, p=1)
    parts['recon_x_mix'] = model.compute_recon_loss_x_mix_list(x_list, xmix, mask, p=1)
    loss = loss + lam['recon_x'] * parts['recon_x'] + lam['recon_x_mix'] * parts['recon_x_mix']
    s_new = model.compute_anatomy_encoding(xf, mask_img)
    _, mu_new, _ = model.compute_modality_encoding(xf, s_new, phase='train')
    parts['latent_z'] = model.compute_latent_z_loss(mu_list, mu_new, mask)
    loss = loss + lam['latent_z'] * parts['latent_z']
    parts['sim_s'] = model.compute_similarity_s_loss(s_list, mask)
    loss = loss + lam['sim_s'] * parts['sim_s']
    parts['sim_z'] = model.compute_similarity_z_loss(z_list, mask)
    loss = loss + lam['sim_z'] * parts['sim_z']
    loss.backward()
    grad_norms = {n: float(p.grad.double().norm()) for n, p in model.named_parameters() if p.grad is not None}
    gnorm = float(torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0))
    opt.step(); opt.zero_grad()
    w1 = {k: float(v.double().sum()) for k, v in model.state_dict().items() if k.startswith(prefixes) and v.dtype.is_floating_point}
    meta = dict(B=B, M=M, H=H, W=W, drop=False, adv=False, lambdas=lam, target_model_name=decoder, fuse_method=fuse,
                dataset_name='BraTS' if brats else 'ZeroDose', norm_type='z-score' if brats else 'mean', out_num_ch=out_num_ch,
                target_seed=TARGET_SEED, loss=float(loss), parts={k: float(v) for k, v in parts.items()},
                grad_norm=gnorm, n_params_with_grad=len(grad_norms), torch=torch.__version__)
    with open(os.path.join(G.OUT, f'step_{tag}.json'), 'w') as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    # the per-parameter records (several hundred names each) go into the .npz with the arrays: name and value columns
    gk, wk = sorted(grad_norms), sorted(w0)
    arrs = dict(y0_pool8=G.pool8(y_list[0].detach()), y1_pool8=G.pool8(y_list[-1].detach()),
                grad_names=np.array(gk), grad_norms=np.array([grad_norms[k] for k in gk]),
                wsum_names=np.array(wk), wsum_before=np.array([w0[k] for k in wk]), wsum_after=np.array([w1[k] for k in wk]))
    np.savez_compressed(os.path.join(G.OUT, f'step_{tag}.npz'), **arrs)
    print(f'step_{tag}: loss={float(loss):.7f} gnorm={gnorm:.4f}', {k: round(float(v), 7) for k, v in parts.items()})


def gen_layout(ref):
    """output_decoder.* state_dict names and shapes of every decoder (fuse_method 'mean', BraTS settings: 4 output channels), in state_dict
    order, and the input channels of down_1 per fuse method: the fuse method changes nothing else (checked here)"""
    layouts, in_ch = {}, {}
    for dec in DECODERS:
        for fuse in FUSE_METHODS:
            torch.manual_seed(10)
            model = build_ref(ref, dec, fuse, True, 4)
            lay = [[k, list(v.shape)] for k, v in model.state_dict().items() if k.startswith('output_decoder.')]
            in_ch.setdefault(fuse, model.output_decoder.down_1[0].in_channels)
            if fuse == 'mean':
                layouts[dec] = lay
            else:
                d1 = 'output_decoder.down_1.0.weight'
                assert [[k, sh] for k, sh in lay if k != d1] == [[k, sh] for k, sh in layouts[dec] if k != d1], (dec, fuse)
    meta = dict(M=M, s_num_ch=4, out_num_ch=4, layouts=layouts, down_1_in_channels=in_ch, torch=torch.__version__)
    with open(os.path.join(G.OUT, 'ckpt_layout_outdec.json'), 'w') as f:
        json.dump(meta, f, sort_keys=True)
    print('ckpt_layout_outdec:', {k: len(v) for k, v in layouts.items()}, in_ch)


def main():
    os.makedirs(G.OUT, exist_ok=True)
    torch.set_num_threads(8)
    ref = G.import_reference()
    for name in sys.argv[1:] or list(FIXTURES):
        step = FIXTURES[name]
        if step is None:
            gen_layout(ref)
        else:
            gen_step(ref, **step)


if __name__ == '__main__':
    main()
