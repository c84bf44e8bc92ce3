"""Golden fixtures for the fully shared input decoder of the reference (config.yaml:65-66 `shared_inp_dec: True`, model.py:3114-3133):
one training step of the real reference model on the CPU per fixture, through oracle/gen_golden.py's own step / layout recorders with
the model constructor swapped for one that passes shared_inp_dec=True (and the fixture's `others`).  Writes new files under
tests/golden/ only; oracle/ is used as it is.

    python tools/gen_golden_shared_dec.py            # all fixtures (a few minutes of CPU)
    python tools/gen_golden_shared_dec.py shdec      # one of them (tags below)
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import gen_golden as G      # noqa: E402

SHIPPED = {'mod_enc_s': False, 'ana_dec_act': 'softmax', 'old': False, 'softmax_remove_mask': True}     # config.yaml:68 (gen_golden's)
ENCS_SOFTPLUS = {'mod_enc_s': True, 'ana_dec_act': 'softplus', 'old': False}                          # config.yaml:70

# tag -> (others, gen_step arguments or None for the checkpoint-layout fixture)
FIXTURES = {
    'shdec': (SHIPPED, dict(tag='b2m2_shdec', B=2, M=2)),
    'shdec_drop': (SHIPPED, dict(tag='b2m4_shdec_drop', B=2, M=4, drop=True, adv=True)),
    'encs_softplus_shdec': (ENCS_SOFTPLUS, dict(tag='b2m2_encs_softplus_shdec', B=2, M=2)),
    'ckpt_shdec': (SHIPPED, None),
}


def shared_dec_builder(others):
    """gen_golden.build_ref_model with shared_inp_dec=True and `others` replaced (same arguments otherwise)"""
    def build(ref, M, adv=False, out_num_ch=1):
        return G.quiet(
            ref.MultimodalModel, input_size=(160, 192), modality_num=M, in_num_ch=7, out_num_ch=out_num_ch,
            s_num_ch=4, z_size=16, is_cond=True, is_discrim_s=adv, is_distri_z=False,
            s_compact_method='max', s_sim_method='cosine', z_sim_method='cosine', shared_ana_enc=True,
            shared_mod_enc=True, shared_inp_dec=True, device=torch.device('cpu'),
            input_output_act='no', target_output_act='no', target_model_name='U+SA', fuse_method='mean',
            others=dict(others))
    return build


def main():
    os.makedirs(G.OUT, exist_ok=True)
    torch.set_num_threads(8)
    ref = G.import_reference()
    only = sys.argv[1:] or list(FIXTURES)
    shipped = G.build_ref_model
    try:
        for name in only:
            others, step = FIXTURES[name]
            G.build_ref_model = shared_dec_builder(others)
            if step is None:
                G.gen_ckpt_layout(ref, tag='ckpt_layout_m2_shdec')
            else:
                G.gen_step(ref, **step)
    finally:
        G.build_ref_model = shipped


if __name__ == '__main__':
    main()
