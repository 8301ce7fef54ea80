"""CPU: the numpy oracle's rectangular geometry (images with H != W, kh x kw kernels, per-axis stride and padding)
against torch on the CPU.

Everything in the oracle after the unfold acts on [B, P, K] and does not depend on the geometry, so pinning unfold,
fold and one exact end-to-end forward pins the generalisation; the golden tests pin the square case to the reference.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cim_oracle as co

# (B, C, H, W, (kh, kw), (sh, sw), (ph, pw)): the anisotropic shapes of test_gpu_rect.py's function cases and two
# plain H != W ones
SHAPES = [
    (2, 16, 8, 16, (1, 3), (1, 1), (0, 1)),
    (2, 16, 8, 16, (3, 1), (1, 1), (1, 0)),
    (2, 16, 8, 32, (3, 3), (1, 2), (1, 1)),
    (2, 16, 16, 16, (3, 3), (2, 1), (1, 1)),
    (2, 16, 10, 16, (3, 3), (1, 1), (0, 1)),
    (2, 16, 7, 5, (3, 2), (2, 1), (1, 0)),
    (2, 16, 5, 7, (3, 3), (1, 1), (1, 1)),
    (3, 4, 12, 32, (3, 3), (1, 1), (1, 1)),
]
IDS = ["%dx%d_k%dx%d_s%d%d_p%d%d" % (s[2], s[3], *s[4], *s[5], *s[6]) for s in SHAPES]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_unfold_equals_torch(shape):
    B, C, H, W, k, s, p = shape
    x = np.random.default_rng(1).integers(-8, 8, size=(B, C, H, W)).astype(np.float32)
    ref = F.unfold(torch.from_numpy(x), k, padding=p, stride=s).transpose(1, 2).numpy()
    assert np.array_equal(co.unfold(x, k, p, s), ref)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fold_equals_torch(shape):
    B, C, H, W, k, s, p = shape
    ho, wo = co.out_size(H, k[0], p[0], s[0]), co.out_size(W, k[1], p[1], s[1])
    cols = np.random.default_rng(2).integers(-8, 8, size=(B, C * k[0] * k[1], ho * wo)).astype(np.float64)
    ref = F.fold(torch.from_numpy(cols), (H, W), k, padding=p, stride=s).numpy()
    got = co.fold(cols, (H, W), k, p, s)
    assert got.shape == (B, C, H, W) and np.array_equal(got, ref)


def test_int_kernel_is_the_square_kernel():
    x = np.random.default_rng(3).integers(0, 8, size=(2, 3, 6, 9)).astype(np.float32)
    assert np.array_equal(co.unfold(x, 3, (1, 1), (1, 2)), co.unfold(x, (3, 3), (1, 1), (1, 2)))
    cols = np.random.default_rng(4).integers(0, 8, size=(2, 27, 6 * 5)).astype(np.float64)
    assert np.array_equal(co.fold(cols, (6, 9), 3, (1, 1), (1, 2)), co.fold(cols, (6, 9), (3, 3), (1, 1), (1, 2)))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_forward_without_adc_equals_conv2d(shape):
    """adc_bits = 0 and power-of-two scales: x_int, w_int and every partial sum are exact small integers (below 2^11,
    exact in fp16), the products by sw * sa and the binary weights exact in fp32, so the oracle's output is the
    float64 convolution of the same x_q, w_q -- equal, not close.  The backward then has the shapes of its inputs."""
    B, C, H, W, k, s, p = shape
    O, bits, xbar = 8, 3, 64
    rng = np.random.default_rng(5)
    sa, sw = np.array([0.125], np.float32), np.array([0.0625], np.float32)
    x_q = (rng.integers(0, 2 ** bits, size=(B, C, H, W)).astype(np.float32) * sa).astype(np.float32)
    qn, qp = co.lsq_weight_params(bits)
    w_q = (rng.integers(qn, qp + 1, size=(O, C) + k).astype(np.float32) * sw).astype(np.float32)
    bm = co.make_binary_mask(bits, bits, 1, 1)
    out, ctx = co.cim_forward(x_q, w_q, s, p, (1, 1), bits, 1, bits, 1, 0, xbar, bm, None, sw, sa, False,
                              np.zeros(1, np.float32))
    ref = F.conv2d(torch.from_numpy(x_q).double(), torch.from_numpy(w_q).double(), None, s, p)
    ref = ref.flatten(2).transpose(1, 2).numpy()
    assert out.shape == ref.shape
    assert np.abs(out.astype(np.float64) - ref).max() == 0.0
    g = rng.standard_normal(out.shape).astype(np.float32)
    gx, gw, ga = co.cim_backward(ctx, g)
    assert gx.shape == x_q.shape and gw.shape == w_q.shape and ga is None


def test_alpha_cim_init_takes_a_rectangular_kernel():
    rng = np.random.default_rng(6)
    sa, sw = np.array([0.125], np.float32), np.array([0.0625], np.float32)
    x_q = (rng.integers(0, 8, size=(2, 16, 7, 5)).astype(np.float32) * sa).astype(np.float32)
    w_q = (rng.integers(-4, 4, size=(24, 16, 3, 2)).astype(np.float32) * sw).astype(np.float32)
    a = co.alpha_cim_init(x_q, w_q, (2, 1), (1, 0), 3, 1, 3, 1, 64, sw, sa, 1.5)
    assert a.shape == (1, 2, 3, 3, 1, 24) and (a > 0).all()
    u = co.analog_partial_sums(x_q, w_q, (2, 1), (1, 0), 3, 1, 3, 1, 64, sw, sa)
    assert u.shape == (2, 2, 3, 3, 4 * 4, 24)
