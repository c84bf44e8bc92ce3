"""The output decoders 'U', 'U+SA', 'U+SA+CA' and 'U+SSA+CA' with every fuse method, built on the CPU (no kernels run): parameter names and
shapes against the reference's layout (tools/gen_golden_outdec.py), seeded inits against the step goldens, the softplus target activation
of a non-BraTS config, and the constructor's refusals."""
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

import mrdis
from fixtures_outdec import DECODERS, FUSE_METHODS

CPU = torch.device('cpu')
SHIPPED_OTHERS = {'mod_enc_s': False, 'ana_dec_act': 'softmax', 'old': False, 'softmax_remove_mask': True}


def _model(decoder, fuse, act='no', out_num_ch=4, target_act=None):
    return mrdis.MultimodalModel(input_size=(160, 192), modality_num=2, in_num_ch=7, out_num_ch=out_num_ch, s_num_ch=4, z_size=16,
                                 shared_ana_enc=True, shared_mod_enc=True, shared_inp_dec=False, device=CPU, input_output_act=act,
                                 target_output_act=target_act or act, target_model_name=decoder, fuse_method=fuse, others=dict(SHIPPED_OTHERS),
                                 build_output_decoder=True)


def _cfg(**kw):
    cfg = dict(mrdis.DEFAULT_CONFIG)
    cfg.update(contrast_list=['m0', 'm1'], input_height=160, input_width=192, batch_size=16, lambda_recon_y=1.0, out_num_ch=4)
    cfg.update(kw)
    return mrdis.derive_config(cfg, CPU)


@pytest.mark.parametrize('fuse', FUSE_METHODS)
@pytest.mark.parametrize('decoder', DECODERS)
def test_output_decoder_layout_matches_the_reference(golden_dir, decoder, fuse):
    meta = json.load(open(os.path.join(golden_dir, 'ckpt_layout_outdec.json')))
    want = [[k, list(sh)] for k, sh in meta['layouts'][decoder]]
    d1 = 'output_decoder.down_1.0.weight'                         # the fuse method sets down_1's input channels, nothing else
    want = [[k, [sh[0], meta['down_1_in_channels'][fuse]] + sh[2:] if k == d1 else sh] for k, sh in want]
    model = _model(decoder, fuse)
    got = [[k, list(v.shape)] for k, v in model.state_dict().items() if k.startswith('output_decoder.')]
    assert got == want


@pytest.mark.parametrize('tag', ['b2m2_u', 'b2m2_uca', 'b2m2_ussaca', 'b2m2_ussaca_sp'])
def test_seeded_init_matches_the_reference(golden_dir, tag):
    """torch.manual_seed(10) before the constructor gives the reference's weights (build order and parameter names as model.py:2951-2964)"""
    meta = json.load(open(os.path.join(golden_dir, f'step_{tag}.json')))
    arrs = np.load(os.path.join(golden_dir, f'step_{tag}.npz'))
    wsum = dict(zip(arrs['wsum_names'].tolist(), arrs['wsum_before'].tolist()))
    act = 'no' if meta['dataset_name'] == 'BraTS' else 'softplus'
    torch.manual_seed(10); np.random.seed(10)
    model = _model(meta['target_model_name'], meta['fuse_method'], act, meta['out_num_ch'])
    sd = model.state_dict()
    keys = [k for k in wsum if k.startswith('output_decoder.')]
    assert keys and set(keys) == {k for k in sd if k.startswith('output_decoder.') and sd[k].dtype.is_floating_point}
    for k, v in wsum.items():
        got = float(sd[k].double().sum())
        assert abs(got - v) <= 1e-6 * max(1.0, abs(v)), k


def test_non_brats_mean_config_builds_a_softplus_decoder():
    """main_missing.py:75-79: a dataset other than BraTS with norm_type 'mean' gets target_output_act 'softplus'"""
    cfg = _cfg(dataset_name='ZeroDose', norm_type='mean', target_model_name='U+SSA+CA', fuse_method='mean-max-min', out_num_ch=1)
    assert cfg['target_output_act'] == 'softplus' and cfg['input_output_act'] == 'softplus'
    model = mrdis.build_model(cfg)
    assert isinstance(model.output_decoder.output_act, nn.Softplus)
    assert model.output_decoder.down_1[0].in_channels == 3 * cfg['s_num_ch']
    for name in DECODERS:
        m = mrdis.build_model(dict(cfg, target_model_name=name, fuse_method='mean'))
        assert isinstance(m.output_decoder.output_act, nn.Softplus), name


def test_unknown_decoder_and_bf16_storage_raise():
    with pytest.raises(ValueError):
        _model('U+SSA', 'mean')
    with pytest.raises(ValueError):
        _model('U', 'median')
    for name in DECODERS:
        mrdis.ops.set_compute_dtype('bf16')
        try:
            with pytest.raises(NotImplementedError, match=name.replace('+', r'\+')):
                mrdis.build_model(_cfg(target_model_name=name, compute_dtype='bf16'))
        finally:
            mrdis.ops.set_compute_dtype('f32')
    with pytest.raises(NotImplementedError):
        _model('U+SA+CA', 'mean', target_act='sigmoid')


def test_outdec_families_are_outside_the_kernel_families():
    fams = mrdis.hip.OUTDEC_FAMILIES
    assert fams == ('chatt', 'symdiff', 'rgate')
    assert not set(fams) & set(mrdis.hip.KERNEL_FAMILIES)
    assert not set(fams) & set(mrdis.hip.VARIANT_FAMILIES + mrdis.hip.LATENT_FAMILIES + mrdis.hip.CONV3D_FAMILIES)
    for name in ('mrdis_chatt_fwd', 'mrdis_chatt_bwd', 'mrdis_symdiff_fwd', 'mrdis_symdiff_bwd', 'mrdis_rgate_fwd', 'mrdis_rgate_bwd'):
        assert name in mrdis.hip.EXPORTED_SYMBOLS
