"""The element-wise float64 bound of tests/conv_check.py against the max-scaled close() of tests/test_gpu_ops.py, on the CPU: faults planted into a
float64 convolution result that a wrong tail mask or a mis-offset epilogue would produce are caught by the new bound and passed by close() at the
rtol the suite uses for that dtype; clean fp32- and bf16-rounded results pass the new bound (it is not vacuous); a coarse fault fails both.
The 3-D references (fwd_ref3d, dgrad_ref3d, wgrad_ref3d) get the same treatment, plus a tap lost on one depth face of the volume."""
import pytest
import torch

import conv_check as CC
from test_gpu_ops import close

KAPPA = 64          # a stand-in for the per-kernel constants of tests/conv_check.py (1 .. 25 outside the F(4x4) Winograd forms and c4_mixed)
RTOL = {'fp32': 1e-4, 'bf16': 1.5e-2}          # what tests/test_gpu_ops.py uses today for these results


def layer(Ci, Co=40, N=2, H=9, W=11, seed=0, bf16=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Ci, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Co, Ci, 3, 3, generator=g, dtype=torch.float64) * (9 * Ci) ** -0.5
    b = torch.randn(Co, generator=g, dtype=torch.float64) * 0.1
    if bf16:
        x, w = CC.bf16_round(x), CC.bf16_round(w)
    ref, A = CC.fwd_ref(x, w, b, 1, 1)
    return x, w, b, ref, A


def stored(ref, dtype):
    """the float64 result as a kernel would store it"""
    return CC.bf16_round(ref) if dtype == 'bf16' else ref.float().double()


def new_check_catches(got, ref, A, dtype):
    with pytest.raises(AssertionError):
        CC.check(got, ref, A, KAPPA, u_out=CC.U_BF16 if dtype == 'bf16' else 0.0, what='planted fault')


@pytest.mark.parametrize('dtype,Ci', [('fp32', 16), ('fp32', 512), ('bf16', 512)])
def test_clean_results_pass_the_bound(dtype, Ci):
    x, w, b, ref, A = layer(Ci, bf16=dtype == 'bf16')
    r = CC.check(stored(ref, dtype), ref, A, KAPPA, u_out=CC.U_BF16 if dtype == 'bf16' else 0.0, what='clean')
    assert r <= 1.0, r                   # storing the exact result costs at most one unit of u A (fp32) / nothing beyond u_out |ref| (bf16)
    ref_l, _ = CC.fwd_ref(x, w, b, 1, 1, lrelu=True)
    CC.check(stored(ref_l, dtype), ref_l, A, KAPPA, u_out=CC.U_BF16 if dtype == 'bf16' else 0.0, what='clean + LeakyReLU')


@pytest.mark.parametrize('dtype,Ci,scale', [('bf16', 512, 2e-2), ('fp32', 16, 1e-4), ('fp32', 512, 1e-4)])
def test_cout_tail_fault_caught_by_the_bound_missed_by_close(dtype, Ci, scale):
    """the last 8 couts of a Co = 40 result scaled by 1 + scale: a wrong tail mask / a mis-offset epilogue"""
    _, _, _, ref, A = layer(Ci, bf16=dtype == 'bf16')
    got = stored(ref, dtype).clone()
    got[:, -8:] *= 1 + scale
    close(got, ref, rtol=RTOL[dtype], what='close() passes the fault')
    new_check_catches(got, ref, A, dtype)


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_dropped_tap_caught_by_both(dtype):
    """the centre tap of the last 8-channel chunk dropped on the top border row (a tap that reads real data, not the zero padding)"""
    Ci = 512
    x, w, b, ref, A = layer(Ci, bf16=dtype == 'bf16', H=6, W=6, Co=40)
    lost = torch.einsum('nch,oc->noh', x[:, -8:, 0, :], w[:, -8:, 1, 1])            # (N, Co, W): what the centre tap adds to row 0
    got = stored(ref, dtype).clone()
    got[:, :, 0, :] -= lost
    new_check_catches(got, ref, A, dtype)
    with pytest.raises(AssertionError):
        close(got, ref, rtol=RTOL[dtype], what='coarse fault')


def test_nan_and_misplaced_elements_fail():
    _, _, _, ref, A = layer(16)
    got = ref.clone(); got[0, 3, 4, 5] = float('nan')
    with pytest.raises(AssertionError):
        CC.check(got, ref, A, KAPPA)
    assert CC.ratio(got, ref, A) == float('inf')
    got = ref.clone(); got[1, 0] = ref[1, 1]
    with pytest.raises(AssertionError):
        CC.check(got, ref, A, KAPPA)


def test_reference_gradients_match_autograd():
    """the data- and weight-gradient references are the adjoints of the forward one"""
    g = torch.Generator().manual_seed(3)
    for (Ci, Co, k, s, p, H, W) in [(5, 6, 3, 1, 1, 9, 11), (7, 16, 4, 2, 1, 10, 12), (4, 6, 3, 2, 1, 11, 13)]:
        x = torch.randn(2, Ci, H, W, generator=g, dtype=torch.float64, requires_grad=True)
        w = torch.randn(Co, Ci, k, k, generator=g, dtype=torch.float64, requires_grad=True)
        b = torch.randn(Co, generator=g, dtype=torch.float64, requires_grad=True)
        y = torch.nn.functional.conv2d(x, w, b, s, p)
        dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        y.backward(dy)
        dx, Adx = CC.dgrad_ref(dy, w.detach(), (H, W), s, p)
        dw, Adw, db, Adb = CC.wgrad_ref(x.detach(), dy, k, k, s, p)
        assert torch.allclose(dx, x.grad) and torch.allclose(dw, w.grad) and torch.allclose(db, b.grad)
        assert (Adx >= dx.abs() - 1e-12).all() and (Adw >= dw.abs() - 1e-12).all() and (Adb >= db.abs()).all()


# ---------------------------------------------------------------- 3-D (tests/test_gpu_conv3d_paths.py)
def layer3d(Ci, Co=20, N=2, D=5, H=6, W=7, seed=0, residual=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Ci, D, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Co, Ci, 3, 3, 3, generator=g, dtype=torch.float64) * (27 * Ci) ** -0.5
    b = torch.randn(Co, generator=g, dtype=torch.float64) * 0.1
    res = torch.randn(N, Co, D, H, W, generator=g, dtype=torch.float64) if residual else None
    ref, A = CC.fwd_ref3d(x, w, b, 1, 1, res)
    return x, w, b, ref, A


@pytest.mark.parametrize('Ci,residual', [(16, False), (128, True)])
def test_clean_3d_results_pass_the_bound(Ci, residual):
    _, _, _, ref, A = layer3d(Ci, residual=residual)
    r = CC.check(stored(ref, 'fp32'), ref, A, KAPPA, what='clean 3-D')
    assert r <= 1.0, r


@pytest.mark.parametrize('Ci,residual', [(16, False), (128, True)])
def test_3d_cout_tail_fault_caught_by_the_bound_missed_by_close(Ci, residual):
    """the last 4 couts of a Co = 20 3-D result scaled by 1 + 1e-4: passes the 1e-3 max-scaled check tests/test_gpu_3d.py uses"""
    _, _, _, ref, A = layer3d(Ci, residual=residual)
    got = stored(ref, 'fp32').clone()
    got[:, -4:] *= 1 + 1e-4
    close(got, ref, rtol=1e-3, what='close() passes the fault')
    new_check_catches(got, ref, A, 'fp32')


@pytest.mark.parametrize('face', ['first', 'last'])
def test_3d_tap_dropped_on_a_depth_face_fails_the_bound(face):
    """one depth tap of the last 8 input channels lost on the first (or last) D plane only -- the tap that reads the real neighbouring plane,
    not the zero padding: a wrong depth-halo mask in a box at the volume boundary"""
    Ci = 64
    x, w, b, ref, A = layer3d(Ci, D=6, H=5, W=6)
    d, r, src = (0, 2, 1) if face == 'first' else (-1, 0, -2)        # out plane, depth tap, the input plane that tap reads
    lost = torch.einsum('nchw,oc->nohw', x[:, -8:, src], w[:, -8:, r, 1, 1])
    got = stored(ref, 'fp32').clone()
    got[:, :, d, 1:, :] -= lost[:, :, 1:, :]          # (every row but the first: the fault is confined to part of one face)
    new_check_catches(got, ref, A, 'fp32')


def test_3d_reference_gradients_match_autograd():
    """the 3-D data- and weight-gradient references are the adjoints of the forward one; the fused residual enters ref and A"""
    g = torch.Generator().manual_seed(5)
    for (Ci, Co, s, D, H, W) in [(5, 6, 1, 4, 5, 6), (4, 10, 2, 5, 7, 6), (3, 8, 2, 1, 3, 4)]:
        x = torch.randn(2, Ci, D, H, W, generator=g, dtype=torch.float64, requires_grad=True)
        w = torch.randn(Co, Ci, 3, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
        b = torch.randn(Co, generator=g, dtype=torch.float64, requires_grad=True)
        y = torch.nn.functional.conv3d(x, w, b, s, 1)
        res = torch.randn(y.shape, generator=g, dtype=torch.float64)
        ref, A = CC.fwd_ref3d(x.detach(), w.detach(), b.detach(), s, 1, res)
        assert torch.allclose(ref, y.detach() + res) and (A >= ref.abs() - 1e-12).all()
        dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        y.backward(dy)
        dx, Adx = CC.dgrad_ref3d(dy, w.detach(), (D, H, W), s, 1)
        dw, Adw, db, Adb = CC.wgrad_ref3d(x.detach(), dy, 3, s, 1)
        assert torch.allclose(dx, x.grad) and torch.allclose(dw, w.grad) and torch.allclose(db, b.grad)
        assert (Adx >= dx.abs() - 1e-12).all() and (Adw >= dw.abs() - 1e-12).all() and (Adb >= db.abs()).all()
