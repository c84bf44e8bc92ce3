"""Golden fixtures for the `others` variants of the reference (config.yaml:67-70): one training step of the real reference model on
the CPU per variant, through oracle/gen_golden.py's own step / layout recorders with the model constructor swapped for one that
passes the variant's `others`.  Writes new files under tests/golden/ only; oracle/ is used as it is.

    python tools/gen_golden_variants.py            # all variant fixtures (a few minutes of CPU)
    python tools/gen_golden_variants.py encs       # one of them (tags below)
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import gen_golden as G      # noqa: E402

ENCS_SOFTMAX = {'mod_enc_s': True, 'ana_dec_act': 'softmax', 'old': False}                 # config.yaml:67
SOFTPLUS = {'mod_enc_s': False, 'ana_dec_act': 'softplus', 'old': False}                   # config.yaml:69
ENCS_SOFTPLUS = {'mod_enc_s': True, 'ana_dec_act': 'softplus', 'old': False}               # config.yaml:70

# tag -> (others, gen_step arguments or None for the checkpoint-layout fixture)
FIXTURES = {
    'encs': (ENCS_SOFTMAX, dict(tag='b2m2_encs', B=2, M=2)),
    'softplus': (SOFTPLUS, dict(tag='b2m2_softplus', B=2, M=2)),
    'encs_softplus_drop': (ENCS_SOFTPLUS, dict(tag='b2m4_encs_softplus_drop', B=2, M=4, drop=True)),
    'ckpt_encs': (ENCS_SOFTMAX, None),
}


def variant_builder(others):
    """gen_golden.build_ref_model with `others` replaced (same arguments otherwise, so the seeded initialisation is the shipped one's
    except for the layers whose shapes the variant changes)."""
    def build(ref, M, adv=False, out_num_ch=1):
        return G.quiet(
            ref.MultimodalModel, input_size=(160, 192), modality_num=M, in_num_ch=7, out_num_ch=out_num_ch,
            s_num_ch=4, z_size=16, is_cond=True, is_discrim_s=adv, is_distri_z=False,
            s_compact_method='max', s_sim_method='cosine', z_sim_method='cosine', shared_ana_enc=True,
            shared_mod_enc=True, shared_inp_dec=False, device=torch.device('cpu'),
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
            G.build_ref_model = variant_builder(others)
            if step is None:
                G.gen_ckpt_layout(ref, tag='ckpt_layout_m2_encs')
            else:
                G.gen_step(ref, **step)
    finally:
        G.build_ref_model = shipped


if __name__ == '__main__':
    main()
