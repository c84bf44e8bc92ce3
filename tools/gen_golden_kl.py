"""Golden fixtures for the latent-code options of the reference's loss block: the KL term (lambda_kl, main_missing.py:219-225), the
learned modality prior (is_distri_z, model.py:2902-2914, 2968-2969) and mean compaction (s_compact_method 'mean', model.py:3453-3456).
One training step of the real reference model on the CPU per fixture, recorded like oracle/gen_golden.py's step fixtures (loss parts,
gradient norms of every parameter, weight sums before and after Adam) by a step recorder of its own, because gen_step hard-codes the
loss set.  Uses oracle/gen_golden.py's helpers as they are; writes new files under tests/golden/ only, the same bytes on every run.

    python tools/gen_golden_kl.py              # all fixtures (a few minutes of CPU)
    python tools/gen_golden_kl.py distri       # one of them (tags below)
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
from fixtures import make_inputs, reinit_discriminator      # noqa: E402  (tests/ is on sys.path through gen_golden)

SHIPPED_OTHERS = {'mod_enc_s': False, 'ana_dec_act': 'softmax', 'old': False, 'softmax_remove_mask': True}
DISTRI_SEED = 778          # distri_z is re-initialised from this seed on both sides (see build)

# tag -> (model options, step arguments or None for the checkpoint-layout fixture)
FIXTURES = {
    'kl': (dict(is_distri_z=False, s_compact_method='max'), dict(tag='b2m2_kl', B=2, M=2, lambda_kl=1.0)),
    # seed 10's drop-out mask, [[1, 1, 0, 1], [1, 0, 1, 1]], leaves every contrast present in some row: the reference's KL is finite
    'distri': (dict(is_distri_z=True, s_compact_method='max'), dict(tag='b2m4_distri_drop', B=2, M=4, lambda_kl=1.0, drop=True)),
    'mean': (dict(is_distri_z=False, s_compact_method='mean'), dict(tag='b2m2_mean', B=2, M=2, lambda_kl=0.0)),
    'ckpt_distri': (dict(is_distri_z=True, s_compact_method='max'), None),
}


def builder(is_distri_z, s_compact_method):
    """gen_golden.build_ref_model with is_distri_z / s_compact_method set (same arguments otherwise)"""
    def build(ref, M, adv=False, out_num_ch=1):
        return G.quiet(
            ref.MultimodalModel, input_size=(160, 192), modality_num=M, in_num_ch=7, out_num_ch=out_num_ch,
            s_num_ch=4, z_size=16, is_cond=True, is_discrim_s=adv, is_distri_z=is_distri_z,
            s_compact_method=s_compact_method, s_sim_method='cosine', z_sim_method='cosine', shared_ana_enc=True,
            shared_mod_enc=True, shared_inp_dec=False, device=torch.device('cpu'),
            input_output_act='no', target_output_act='no', target_model_name='U+SA', fuse_method='mean',
            others=dict(SHIPPED_OTHERS))
    return build


def gen_step(ref, build, is_distri_z, tag, B, M, lambda_kl, drop=False):
    """main_missing.py:175-284 for one batch with the shipped loss weights plus lambda_kl: the KL term sits between recon_x_mix and
    latent_z in the loss sum, two-Gaussian under is_distri_z (:219-225)."""
    lam = dict(recon_x=1.0, recon_x_mix=2.0, kl=lambda_kl, latent_z=0.1, sim_s=10.0, sim_z=2.0)
    torch.manual_seed(10); np.random.seed(10)                       # main_missing.py:18-21
    model = build(ref, M)
    prefixes = G.HOT_PREFIXES + (('distri_z.',) if is_distri_z else ())
    if is_distri_z:
        # built behind the output decoder, whose RNG draws the restatement does not make unless lambda_recon_y > 0: a seed-independent init
        reinit_discriminator(model.distri_z, seed=DISTRI_SEED)
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=2e-4, weight_decay=1e-5, amsgrad=True)
    inputs, mask, mask_img = make_inputs(B, M, 160, 192, seed=10, drop=drop)
    torch.manual_seed(11); np.random.seed(11)
    w0 = {k: float(v.double().sum()) for k, v in model.state_dict().items() if k.startswith(prefixes) and v.dtype.is_floating_point}

    x_list = [inputs[:, i * 7:(i + 1) * 7] for i in range(M)]
    s_list = model.compute_anatomy_encoding(x_list, mask_img)
    z_list, mu_list, lv_list = model.compute_modality_encoding(x_list, s_list, phase='train')
    xf = model.reconstruct_input_si_zi(s_list, z_list)
    xmix = model.reconstruct_input_si_zj(s_list, z_list)
    parts = {}
    parts['recon_x'] = model.compute_recon_loss_x_list(x_list, xf, mask, p=1)
    parts['recon_x_mix'] = model.compute_recon_loss_x_mix_list(x_list, xmix, mask, p=1)
    loss = lam['recon_x'] * parts['recon_x'] + lam['recon_x_mix'] * parts['recon_x_mix']
    if lambda_kl > 0:
        if is_distri_z:
            pm_list, plv_list = model.compute_zi_prior_distribution(B, M, torch.device('cpu'))
            parts['kl'] = model.compute_kl_loss_list_two_gaussian(mu_list, lv_list, pm_list, plv_list, mask)
        else:
            parts['kl'] = model.compute_kl_loss_list_standard(mu_list, lv_list, mask)
        loss = loss + lam['kl'] * parts['kl']
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
    compact = {}
    if model.s_compact_method == 'mean':
        compact['s0_compact'] = model.compute_compact_s(s_list[0]).detach().numpy()
    meta = dict(B=B, M=M, H=160, W=192, drop=drop, adv=False, lambdas=lam, is_distri_z=is_distri_z,
                s_compact_method=model.s_compact_method, distri_seed=DISTRI_SEED if is_distri_z else None,
                loss=float(loss), parts={k: float(v) for k, v in parts.items()},
                grad_norm=gnorm, grad_norms=grad_norms, wsum_before=w0, wsum_after=w1,
                n_params_with_grad=len(grad_norms), torch=torch.__version__)
    with open(os.path.join(G.OUT, f'step_{tag}.json'), 'w') as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    arrs = dict(mu=torch.stack(mu_list).detach().numpy(), z=torch.stack(z_list).detach().numpy(),
                lv=torch.stack(lv_list).detach().numpy(),
                s0_pool8=G.pool8(s_list[0].detach()), xf0_pool8=G.pool8(xf[0].detach()),
                xmix0_pool8=G.pool8(xmix[0].detach()), mask=mask.numpy(), **compact)
    np.savez_compressed(os.path.join(G.OUT, f'step_{tag}.npz'), **arrs)
    print(f'step_{tag}: loss={float(loss):.7f} gnorm={gnorm:.4f}', {k: round(float(v), 7) for k, v in parts.items()})


def main():
    os.makedirs(G.OUT, exist_ok=True)
    torch.set_num_threads(8)
    ref = G.import_reference()
    only = sys.argv[1:] or list(FIXTURES)
    shipped = G.build_ref_model
    try:
        for name in only:
            opts, step = FIXTURES[name]
            build = builder(**opts)
            if step is None:
                G.build_ref_model = build
                G.gen_ckpt_layout(ref, tag='ckpt_layout_m2_distri')
            else:
                gen_step(ref, build, opts['is_distri_z'], **step)
    finally:
        G.build_ref_model = shipped


if __name__ == '__main__':
    main()
