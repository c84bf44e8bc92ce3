"""The latent-code options of the reference's loss block without a GPU: lambda_kl, is_distri_z (the learned modality prior) and
s_compact_method 'mean'.  Which settings the model builds, the parameter layout of an is_distri_z model against the real reference's
(tests/golden/ckpt_layout_m2_distri.json, tools/gen_golden_kl.py), the config path, the prior's broadcast, and the launch-counter
names of the new kernels."""
import json
import os

import numpy as np
import pytest
import torch

CPU = torch.device('cpu')


@pytest.fixture(scope='module')
def m():
    import mrdis
    return mrdis


def _args(**kw):
    a = dict(input_size=(64, 64), modality_num=2, s_num_ch=4, shared_ana_enc=True, shared_inp_dec=False, device=CPU,
             others={'mod_enc_s': False, 'ana_dec_act': 'softmax', 'old': False, 'softmax_remove_mask': True}, latent_options=True)
    a.update(kw)
    return a


@pytest.mark.parametrize('kw', [dict(is_distri_z=True), dict(s_compact_method='mean'), dict(is_distri_z=True, s_compact_method='mean')], ids=str)
def test_latent_options_build(m, kw):
    model = m.MultimodalModel(**_args(**kw))
    assert hasattr(model, 'distri_z') == kw.get('is_distri_z', False)
    assert model.s_compact_method == kw.get('s_compact_method', 'max')
    if hasattr(model, 'distri_z'):
        assert list(model.state_dict())[-4:] == ['distri_z.linear.0.weight', 'distri_z.linear.0.bias', 'distri_z.linear.2.weight', 'distri_z.linear.2.bias']
        assert all(p.dtype == torch.float32 for p in model.distri_z.parameters())


@pytest.mark.parametrize('kw', [dict(is_distri_z=True), dict(s_compact_method='mean')], ids=str)
def test_constructor_without_the_opt_in_keeps_its_contract(m, kw):
    """a direct MultimodalModel call without latent_options=True is refused as before (and says how to opt in); build_model opts in"""
    with pytest.raises(NotImplementedError, match='latent_options=True'):
        m.MultimodalModel(**_args(latent_options=False, **kw))
    cfg = dict(m.DEFAULT_CONFIG)
    cfg.update(contrast_list=['a', 'b'], input_height=64, input_width=64, **kw)
    model = m.build_model(m.derive_config(cfg, CPU))
    assert model.is_distri_z == kw.get('is_distri_z', False) and model.s_compact_method == kw.get('s_compact_method', 'max')


@pytest.mark.parametrize('kw', [dict(s_compact_method='vgg'), dict(s_sim_method='perceptual')], ids=str)
def test_vgg_options_name_the_pretrained_weights(m, kw):
    with pytest.raises(NotImplementedError, match='pretrained VGG16'):
        m.MultimodalModel(**_args(**kw))


@pytest.mark.parametrize('kw', [dict(shared_inp_dec=True), dict(z_sim_method='l1'), dict(s_compact_method='median'),
                                dict(others={'mod_enc_s': False, 'ana_dec_act': 'softmax', 'old': True})], ids=str)
def test_out_of_scope_settings_stay_rejected(m, kw):
    with pytest.raises(NotImplementedError, match='only the shipped config.yaml graph is built'):
        m.MultimodalModel(**_args(**kw))


def test_distri_z_checkpoint_layout_matches_reference(m, golden_dir):
    """state_dict of an is_distri_z model = the reference's: every key (distri_z.linear.{0,2}.{weight,bias} included), shape and dtype, and
    the seeded-init sums of everything but discrim_s and distri_z (built behind modules whose draws differ); a checkpoint of that layout loads with nothing skipped"""
    lay = json.load(open(os.path.join(golden_dir, 'ckpt_layout_m2_distri.json')))
    cfg = dict(m.DEFAULT_CONFIG)
    cfg.update(contrast_list=['a', 'b'], is_distri_z=True, lambda_adv_s=1.0, lambda_recon_y=1.0)
    cfg = m.derive_config(cfg, CPU)
    torch.manual_seed(10); np.random.seed(10)
    model = m.build_model(cfg)
    sd = model.state_dict()
    assert set(sd) == set(lay['model'])
    assert lay['model']['distri_z.linear.2.weight']['shape'] == [32, 128]
    fake = {}
    for k, rec in lay['model'].items():
        assert list(sd[k].shape) == rec['shape'] and str(sd[k].dtype).replace('torch.', '') == rec['dtype'], k
        if not k.startswith(('discrim_s.', 'distri_z.')) and sd[k].dtype.is_floating_point:
            assert abs(float(sd[k].double().sum()) - rec['sum']) <= 1e-6 * max(1.0, abs(rec['sum'])), k
        fake[k] = torch.full(rec['shape'], 0.25, dtype=sd[k].dtype)
    assert m.load_checkpoint_model(model, fake) == []
    assert float(model.distri_z.linear[2].weight.detach().sum()) == 0.25 * 32 * 128


def test_distri_z_is_trainable_only_with_the_kl_term(m):
    model = m.MultimodalModel(**_args(is_distri_z=True))
    names = {id(p): n for n, p in model.named_parameters()}
    with_kl = {names[id(p)] for p in model.trainable_parameters()}
    without = {names[id(p)] for p in model.trainable_parameters(with_prior=False)}
    prior = {n for n in with_kl if n.startswith('distri_z.')}
    assert len(prior) == 4 and with_kl - without == prior


def test_prior_is_evaluated_once_and_broadcast(m):
    """compute_zi_prior_distribution: the values of the reference's per-row evaluation (distri_z on (i + 1) * ones(bs, 1))"""
    torch.manual_seed(3)
    model = m.MultimodalModel(**_args(is_distri_z=True, modality_num=3))
    pm, plv = model.compute_zi_prior_distribution(5, 3, CPU)
    assert len(pm) == len(plv) == 3 and all(tuple(t.shape) == (5, 16) for t in pm + plv)
    for i in range(3):
        rm, rlv = model.distri_z((i + 1) * torch.ones(5, 1))
        assert torch.allclose(pm[i], rm, rtol=1e-6, atol=1e-7) and torch.allclose(plv[i], rlv, rtol=1e-6, atol=1e-7)


def test_config_yaml_round_trips_the_latent_keys(m, tmp_path):
    import yaml
    base = dict(contrast_list=['T1', 'T2'], input_height=64, input_width=64, batch_size=4, data_source='synthetic', ckpt_root=str(tmp_path / 'ckpt'),
                ckpt_timelabel='t0', lambda_kl=0.5, is_distri_z=True, s_compact_method='mean')
    (tmp_path / 'config.yaml').write_text(yaml.dump(base))
    cfg = m.train.setup_config(str(tmp_path / 'config.yaml'), device=CPU)
    assert (cfg['lambda_kl'], cfg['is_distri_z'], cfg['s_compact_method']) == (0.5, True, 'mean')
    model = m.build_model(cfg)
    assert model.is_distri_z and model.s_compact_method == 'mean'


def test_gallery_carries_its_compaction_method(m, tmp_path):
    Z = m.trainer.ZGallery
    g = Z(torch.zeros(4, 2, 8), torch.zeros(4, 2, 16), torch.tensor([0, 0, 1, 1], dtype=torch.int32), torch.arange(4), ['a', 'b'], 'mean')
    g2 = Z.load(g.save(str(tmp_path / 'g.pt')), CPU)
    assert g2.compact_method == 'mean'
    d = torch.load(str(tmp_path / 'g.pt'), weights_only=True)
    del d['compact_method']
    torch.save(d, str(tmp_path / 'old.pt'))
    assert Z.load(str(tmp_path / 'old.pt'), CPU).compact_method == 'max'           # galleries from before the tag: max-pooled
    model = m.MultimodalModel(**_args())
    with pytest.raises(ValueError, match="s_compact_method 'mean'"):
        g2.check_compact_method(model)
    with pytest.raises(ValueError, match='not comparable'):
        m.trainer.EvalStep(model, dict(m.DEFAULT_CONFIG), info='nearest_neighbour', gallery=g2)


def test_latent_counter_families_are_known_to_the_library(m):
    lib = m.hip.load()
    for fam in m.hip.LATENT_FAMILIES:
        assert lib.mrdis_launch_count(fam.encode()) >= 0, fam
        assert fam not in m.hip.KERNEL_FAMILIES
    assert set(m.hip.LATENT_FAMILIES) <= set(m.hip.launch_counts())


def test_latent_goldens_are_present(golden_dir):
    for tag, key in (('b2m2_kl', 'kl'), ('b2m4_distri_drop', 'kl'), ('b2m2_mean', 'sim_s')):
        meta = json.load(open(os.path.join(golden_dir, f'step_{tag}.json')))
        assert key in meta['parts'] and np.isfinite(meta['loss'])
        assert os.path.exists(os.path.join(golden_dir, f'step_{tag}.npz'))
    meta = json.load(open(os.path.join(golden_dir, 'step_b2m4_distri_drop.json')))
    assert {f'distri_z.linear.{k}' for k in ('0.weight', '0.bias', '2.weight', '2.bias')} <= set(meta['grad_norms'])
    assert (np.load(os.path.join(golden_dir, 'step_b2m4_distri_drop.npz'))['mask'].sum(0) > 0).all()
