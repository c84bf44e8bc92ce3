"""The fully shared input decoder of the reference (config.yaml `shared_inp_dec: True`, SPADENew, model.py:2490-2538) without a GPU:
which settings build it, its parameter layout against the real reference's checkpoint layout (tests/golden/ckpt_layout_m2_shdec.json,
tools/gen_golden_shared_dec.py), and the step plumbing that depends on the decoder topology (mixing groups, gradient-arena order,
Adam gates)."""
import json
import os

import numpy as np
import pytest
import torch

CPU = torch.device('cpu')
SHIPPED = {'mod_enc_s': False, 'ana_dec_act': 'softmax', 'old': False, 'softmax_remove_mask': True}


@pytest.fixture(scope='module')
def m():
    import mrdis
    return mrdis


def _cfg(m, **kw):
    cfg = dict(m.DEFAULT_CONFIG)
    cfg.update(contrast_list=['a', 'b'], input_height=64, input_width=64, shared_inp_dec=True)
    cfg.update(kw)
    return m.derive_config(cfg, CPU)


def _args(**kw):
    a = dict(input_size=(64, 64), modality_num=2, s_num_ch=4, shared_ana_enc=True, shared_inp_dec=True, device=CPU, others=dict(SHIPPED))
    a.update(kw)
    return a


def test_shared_decoder_checkpoint_layout_matches_reference(m, golden_dir):
    """build_model with shared_inp_dec: True builds ONE SPADENew whose state_dict is the reference's: every key, shape, dtype and
    seeded-init sum; a checkpoint of that layout loads with nothing skipped"""
    lay = json.load(open(os.path.join(golden_dir, 'ckpt_layout_m2_shdec.json')))
    cfg = _cfg(m, input_height=160, input_width=192, lambda_adv_s=1.0, lambda_recon_y=1.0)
    torch.manual_seed(10); np.random.seed(10)
    model = m.build_model(cfg)
    assert len(model.input_decoder_list) == 1 and type(model.input_decoder_list[0]) is m.SPADENew
    sd = model.state_dict()
    assert set(sd) == set(lay['model'])
    dec_keys = [k for k in lay['model'] if k.startswith('input_decoder_list.')]
    assert len(dec_keys) == 102 and all(k.startswith('input_decoder_list.0.') for k in dec_keys)
    assert sum(int(np.prod(lay['model'][k]['shape'])) for k in dec_keys) == 5566589
    fake = {}
    for k, rec in lay['model'].items():
        assert list(sd[k].shape) == rec['shape'] and str(sd[k].dtype).replace('torch.', '') == rec['dtype'], k
        if not k.startswith('discrim_s.') and sd[k].dtype.is_floating_point:
            assert abs(float(sd[k].double().sum()) - rec['sum']) <= 1e-6 * max(1.0, abs(rec['sum'])), k
        fake[k] = torch.full(rec['shape'], 0.25, dtype=sd[k].dtype)
    assert m.load_checkpoint_model(model, fake) == []
    assert float(model.input_decoder_list[0].out.weight.detach().sum()) == 0.25 * model.input_decoder_list[0].out.weight.numel()


def test_submodule_order_is_the_reference_construction_order(m):
    dec = m.SPADENew((64, 64), 7, 16, 128, 4, True, 'softplus')
    assert [n for n, _ in dec.named_children()] == ['zi_scaler', 'sp1', 'sp2', 'sp3', 'sp4', 'sp5', 'sp6', 'out', 'out_act']
    assert isinstance(dec.out_act, torch.nn.Softplus)
    assert isinstance(m.SPADENew((64, 64), output_activation='no').out_act, torch.nn.Sequential)
    with pytest.raises(ValueError):
        m.SPADENew((64, 64), output_activation='sigmoid')
    assert tuple(dec.out.weight.shape) == (3, 7, 16, 1, 1) and tuple(dec.zi_scaler.weight.shape) == (64 * 64 * 128 // 1024, 16)


@pytest.mark.parametrize('kw', [{}, dict(latent_options=True)], ids=['plain', 'latent_options'])
def test_constructor_without_the_opt_in_keeps_its_contract(m, kw):
    """a direct MultimodalModel(shared_inp_dec=True) call without decoder_options=True is refused as before (and says how to opt in)"""
    with pytest.raises(NotImplementedError, match='only the shipped config.yaml graph is built') as e:
        m.MultimodalModel(**_args(**kw))
    assert 'decoder_options=True' in str(e.value)
    model = m.MultimodalModel(**_args(decoder_options=True, **kw))
    assert model.shared_inp_dec and type(model.input_decoder_list[0]).__name__ == 'SPADENew'


@pytest.mark.parametrize('kw', [dict(others={'mod_enc_s': False, 'ana_dec_act': 'softmax', 'old': True}), dict(s_sim_method='l2'),
                                dict(z_sim_method='l1'), dict(s_compact_method='vgg')], ids=str)
def test_out_of_scope_settings_stay_rejected_with_the_opt_in(m, kw):
    with pytest.raises(NotImplementedError):
        m.MultimodalModel(**_args(decoder_options=True, latent_options=True, **kw))


def test_bf16_storage_is_refused(m):
    with pytest.raises(NotImplementedError, match='shared_inp_dec'):
        m.build_model(_cfg(m, compute_dtype='bf16'))
    m.ops.set_compute_dtype('f32')
    assert m.build_model(_cfg(m, compute_dtype='bf16m')).shared_inp_dec
    m.ops.set_compute_dtype('f32')


@pytest.mark.parametrize('M', [2, 4])
def test_step_plumbing_follows_the_topology(m, M):
    model = m.build_model(_cfg(m, contrast_list=[str(i) for i in range(M)], lambda_adv_s=1.0, lambda_recon_y=1.0, is_distri_z=True,
                               lambda_kl=1.0))
    dec = model.input_decoder_list[0]
    assert [n for n, _ in model.mix_groups()] == ['enc', 'dec'] and model.mix_groups()[1][1] == [dec]
    groups = model.completion_groups()
    ids = [id(p) for g in groups for p in g]
    assert len(ids) == len(set(ids)) and set(ids) == {id(p) for p in model.parameters()}
    assert [id(p) for p in groups[0]] == [id(p) for p in dec.parameters()]
    assert model.gated_parameter_groups() == []
    mask = np.ones((2, M), np.float32); mask[0, 0] = 0
    assert model.active_decoders(mask).tolist() == [1.0]
    assert model.active_decoders(np.zeros((2, M), np.float32)).tolist() == [0.0]


def test_split_topology_is_unchanged(m):
    model = m.build_model(_cfg(m, shared_inp_dec=False))
    assert [n for n, _ in model.mix_groups()] == ['enc', 'dec_shared', 'dec0', 'dec1']
    assert len(model.gated_parameter_groups()) == 2 and len(model.completion_groups()) == 4


def test_arena_optimizer_takes_the_shared_grouping(m):
    """ArenaAdam over the shared-decoder model: the arena is laid out decoder first, and set_gates([]) leaves no gate"""
    model = m.build_model(_cfg(m))
    used = model.trainable_parameters(with_prior=False)
    opt = m.ArenaAdam(model.parameters(), lr=2e-4, weight_decay=1e-5, used=used, order=model.completion_groups())
    opt.set_gates(model.gated_parameter_groups())
    assert opt.n_flags == 0 and not opt.gate_ranges
    dec_ids = {id(p) for p in model.input_decoder_list[0].parameters()}
    assert all(id(p) in dec_ids for p in opt.used[:len(dec_ids)])


def test_config_yaml_key_reaches_the_model(m, tmp_path):
    import yaml
    base = dict(contrast_list=['T1', 'T2'], input_height=64, input_width=64, batch_size=4, data_source='synthetic',
                ckpt_root=str(tmp_path / 'ckpt'), ckpt_timelabel='t0', shared_inp_dec=True)
    (tmp_path / 'config.yaml').write_text(yaml.dump(base))
    cfg = m.train.setup_config(str(tmp_path / 'config.yaml'), device=CPU)
    assert cfg['shared_inp_dec'] is True
    assert m.build_model(cfg).shared_inp_dec


def test_shared_decoder_goldens_are_present(golden_dir):
    for tag in ('b2m2_shdec', 'b2m4_shdec_drop', 'b2m2_encs_softplus_shdec'):
        meta = json.load(open(os.path.join(golden_dir, f'step_{tag}.json')))
        assert 'input_decoder_list.0.sp6.out.weight' in meta['grad_norms']
        assert not any(k.startswith('input_decoder_list.1.') for k in meta['grad_norms'])
        assert os.path.getsize(os.path.join(golden_dir, f'step_{tag}.npz')) < 100_000
