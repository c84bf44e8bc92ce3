"""The `others` variants of the reference (config.yaml:67-70) without a GPU: which settings the model builds, the parameter layout of a
mod_enc_s model against the real reference's checkpoint layout (tests/golden/ckpt_layout_m2_encs.json, tools/gen_golden_variants.py),
the config path, and the launch-counter names of the new kernels."""
import json
import os

import numpy as np
import pytest
import torch

CPU = torch.device('cpu')
SIX = [dict(mod_enc_s=e, ana_dec_act=a, old=False, **({'softmax_remove_mask': True} if rm else {}))
       for e in (False, True) for (a, rm) in (('softmax', True), ('softmax', False), ('softplus', False))]


@pytest.fixture(scope='module')
def m():
    import mrdis
    return mrdis


def _cfg(m, others, **kw):
    cfg = dict(m.DEFAULT_CONFIG)
    cfg.update(contrast_list=['a', 'b'], input_height=64, input_width=64, others=others)
    cfg.update(kw)
    return m.derive_config(cfg, CPU)


@pytest.mark.parametrize('others', SIX, ids=lambda o: f"encs{int(o['mod_enc_s'])}_{o['ana_dec_act']}{'_drop' if 'softmax_remove_mask' in o else ''}")
def test_six_variants_build(m, others):
    model = m.build_model(_cfg(m, others))
    enc = model.modality_encoder_list[0]
    assert model.modality_encoder_reads_s() == others['mod_enc_s']
    assert tuple(enc.conv1.weight.shape) == (3, 16, 7 + (4 if others['mod_enc_s'] else 0), 3, 3)
    assert ('mod_enc_s' in model.variant) == others['mod_enc_s']


def test_reference_default_others_is_mod_enc_s_softmax(m):
    """the reference constructor's default others = {'mod_enc_s': True, 'ana_dec_act': 'softmax'} (model.py:2921): builds, reads s"""
    model = m.MultimodalModel(input_size=(64, 64), modality_num=2, s_num_ch=4, shared_ana_enc=True, shared_inp_dec=False, device=CPU)
    assert model.modality_encoder_reads_s() and model.variant == 'mod_enc_s+softmax'
    with pytest.raises(ValueError, match='need_maps'):
        model.compute_anatomy_encoding([torch.zeros(1, 7, 64, 64)] * 2, None, need_maps=False)


@pytest.mark.parametrize('kw', [dict(others={'mod_enc_s': False, 'ana_dec_act': 'softmax', 'old': True}), dict(is_distri_z=True),
                                dict(shared_inp_dec=True), dict(s_compact_method='mean'), dict(s_sim_method='l2'), dict(z_sim_method='l1'),
                                dict(others={'mod_enc_s': True, 'ana_dec_act': 'sigmoid'})], ids=str)
def test_everything_else_stays_rejected(m, kw):
    args = dict(input_size=(64, 64), modality_num=2, s_num_ch=4, shared_ana_enc=True, shared_inp_dec=False, device=CPU,
                others={'mod_enc_s': False, 'ana_dec_act': 'softmax', 'old': False, 'softmax_remove_mask': True})
    args.update(kw)
    with pytest.raises(NotImplementedError, match='only the shipped config.yaml graph is built'):
        m.MultimodalModel(**args)


def test_mod_enc_s_checkpoint_layout_matches_reference(m, golden_dir):
    """state_dict of a mod_enc_s model = the reference's for that variant: every key, shape, dtype and seeded-init sum (conv1 weight
    (3, 16, 11, 3, 3)); a checkpoint of that layout loads with nothing skipped"""
    lay = json.load(open(os.path.join(golden_dir, 'ckpt_layout_m2_encs.json')))
    cfg = _cfg(m, {'mod_enc_s': True, 'ana_dec_act': 'softmax', 'old': False}, input_height=160, input_width=192,
               lambda_adv_s=1.0, lambda_recon_y=1.0)
    torch.manual_seed(10); np.random.seed(10)
    model = m.build_model(cfg)
    sd = model.state_dict()
    assert set(sd) == set(lay['model'])
    assert lay['model']['modality_encoder_list.0.conv1.weight']['shape'] == [3, 16, 11, 3, 3]
    fake = {}
    for k, rec in lay['model'].items():
        assert list(sd[k].shape) == rec['shape'] and str(sd[k].dtype).replace('torch.', '') == rec['dtype'], k
        if not k.startswith('discrim_s.') and sd[k].dtype.is_floating_point:
            assert abs(float(sd[k].double().sum()) - rec['sum']) <= 1e-6 * max(1.0, abs(rec['sum'])), k
        fake[k] = torch.full(rec['shape'], 0.25, dtype=sd[k].dtype)
    assert m.load_checkpoint_model(model, fake) == []
    names = {id(p): n for n, p in model.named_parameters()}
    assert 'modality_encoder_list.0.conv1.weight' in {names[id(p)] for p in model.trainable_parameters()}


def test_config_yaml_others_reaches_the_model(m, tmp_path):
    import yaml
    others = {'mod_enc_s': True, 'ana_dec_act': 'softplus', 'old': False}
    base = dict(contrast_list=['T1', 'T2'], input_height=64, input_width=64, batch_size=4, data_source='synthetic',
                ckpt_root=str(tmp_path / 'ckpt'), ckpt_timelabel='t0', others=others)
    (tmp_path / 'config.yaml').write_text(yaml.dump(base))
    cfg = m.train.setup_config(str(tmp_path / 'config.yaml'), device=CPU)
    assert cfg['others'] == others
    assert m.build_model(cfg).variant == 'mod_enc_s+softplus'


def test_variant_counter_families_are_known_to_the_library(m):
    lib = m.hip.load()
    for fam in m.hip.VARIANT_FAMILIES:
        assert lib.mrdis_launch_count(fam.encode()) >= 0, fam
        assert fam not in m.hip.KERNEL_FAMILIES
    assert lib.mrdis_conv2d_2src_bwd_weight_workspace(32, 256, 256, 7, 4, 16, 3, 3, 2, 1) > 0
    assert lib.mrdis_conv2d_2src_bwd_weight_workspace(2, 8, 8, 7, 30, 16, 3, 3, 2, 1) == 0          # Cx + Cs > 32: unsupported


def test_variant_goldens_are_present(golden_dir):
    for tag in ('b2m2_encs', 'b2m2_softplus', 'b2m4_encs_softplus_drop'):
        meta = json.load(open(os.path.join(golden_dir, f'step_{tag}.json')))
        assert 'modality_encoder_list.0.conv1.weight' in meta['grad_norms']
        assert os.path.exists(os.path.join(golden_dir, f'step_{tag}.npz'))


@pytest.mark.parametrize('value,reads_s', [(False, False), (0, False), (np.bool_(False), False), (True, True), (None, True), ('missing', True)],
                         ids=['False', 'int0', 'numpy_False', 'True', 'None', 'missing'])
def test_mod_enc_s_is_read_as_the_reference_reads_it(m, value, reads_s):
    """model.py:2993 / :3104: s_num_ch = 0 exactly when 'mod_enc_s' in others and others['mod_enc_s'] == False"""
    others = {'ana_dec_act': 'softmax', 'old': False}
    if value != 'missing':
        others['mod_enc_s'] = value
    model = m.MultimodalModel(input_size=(64, 64), modality_num=2, s_num_ch=4, shared_ana_enc=True, shared_inp_dec=False, device=CPU, others=others)
    assert model.modality_encoder_reads_s() == reads_s
