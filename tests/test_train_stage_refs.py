"""Plain NumPy fp64 references of the backward-pass stage kernels (contracts in include/fwn.h), and their proofs
against an independent formulation - fp64 torch.autograd - on the CPU.  tests/test_train_stages.py holds the HIP
kernels to these references; here the references themselves are checked, so that the header's formulas (the edge
taps of the transposed conv, the factor 3 and the constant -3 / (2 Ch) of ActNorm's logs) are not merely assumed.

Every reduction comes with `*_abs`: the same sum over absolute values, per output element - what the tolerance of
a fixed-order fp64 sum of exact fp32 products is derived from."""
import numpy as np
import pytest
import torch


def ref_upsample_bwd(dy, y, x, wk, s, slope=np.float32(0.4)):
    """Backward of y = leaky_relu(conv_transpose(x; wk) + bias, slope), x [B][H][W], wk [2s][3], output row
    tau = i s + k - s/2, column w + kw - 1; rows and columns out of range contribute nothing.
    dpre is computed in dy's own type (fp32 inputs: the bits the kernel must write), everything else in fp64."""
    B, H, W = x.shape
    one = dy.dtype.type(1.0)
    dpre = dy * np.where(y > 0, one, dy.dtype.type(slope))
    assert dpre.dtype == dy.dtype
    P = np.zeros((B, H * s + s, W + 2))                  # row tau at tau + s/2, column ww at ww + 1
    P[:, s // 2:s // 2 + H * s, 1:W + 1] = dpre
    x64, wk64 = x.astype(np.float64), wk.astype(np.float64)
    dx, dx_abs = np.zeros((B, H, W)), np.zeros((B, H, W))
    dw, dw_abs = np.zeros(6 * s + 1), np.zeros(6 * s + 1)
    for k in range(2 * s):
        for kw in range(3):
            tap = P[:, k:k + H * s:s, kw:kw + W]         # dpre[b, i s + k - s/2, w + kw - 1] for every (b, i, w)
            dx += tap * wk64[k, kw]
            dx_abs += np.abs(tap * wk64[k, kw])
            dw[3 * k + kw] = (x64 * tap).sum()
            dw_abs[3 * k + kw] = np.abs(x64 * tap).sum()
    dw[6 * s] = dpre.astype(np.float64).sum()
    dw_abs[6 * s] = np.abs(dpre.astype(np.float64)).sum()
    return dict(dpre=dpre, dx=dx, dx_abs=dx_abs, dwk_bias=dw, dwk_bias_abs=dw_abs)


def ref_small_grads(ga, ya, gb, yb, dzz, an, br, zc):
    """fwn_flow_small_grads: g = dL/dy and y = ActNorm output of both planes [M][Ch], an [2][4][Ch] = (shift, scale,
    1 / scale, 3 logs), dzz [M][2 Ch]; br [Ch] / zc [2 Ch] map device channels to the parameters' order."""
    Ch = ga.shape[1]
    an = an.astype(np.float64)
    out = dict(db=np.zeros(2 * Ch), dlogs=np.zeros(2 * Ch), dzscale=np.zeros(2 * Ch))
    out.update({k + "_abs": np.zeros(2 * Ch) for k in ("db", "dlogs", "dzscale")})
    for role, (g, y) in enumerate(((ga, ya), (gb, yb))):
        g, y = g.astype(np.float64), y.astype(np.float64)
        shift, scale, iscale = an[role, 0], an[role, 1], an[role, 2]
        dst = role * Ch + np.asarray(br)
        out["db"][dst] = g.sum(0) * scale
        out["db_abs"][dst] = np.abs(g).sum(0) * scale
        out["dlogs"][dst] = 3.0 * (g * y).sum(0) - 3.0 / (2.0 * Ch)
        out["dlogs_abs"][dst] = 3.0 * np.abs(g * y).sum(0) + 3.0 / (2.0 * Ch)
        out["g%d" % role] = g * scale
        out["x%d" % role] = y * iscale - shift
        out["x%d_abs" % role] = np.abs(y * iscale) + np.abs(shift)
    z = dzz.astype(np.float64)
    out["dzscale"][np.asarray(zc)] = 3.0 * z.sum(0)
    out["dzscale_abs"][np.asarray(zc)] = 3.0 * np.abs(z).sum(0)
    return out


# The first four shapes of the GPU test (B H <= 120: what fp64 autograd does in well under a second)
@pytest.mark.parametrize("B,H,W,s", [(1, 3, 8, 2), (2, 5, 80, 4), (1, 64, 7, 4), (3, 40, 80, 16)])
def test_upsample_backward_reference_equals_autograd_of_the_transposed_conv(B, H, W, s):
    """The forward is the oracle's own up-sampling stage (oracle/flowavenet_torch.py upsample(): conv_transpose2d with
    stride (s, 1), padding (s // 2, 1) on a [in = 1][out = 1][2s][3] kernel, then leaky_relu(0.4)), fp64; its autograd
    against the NumPy loops."""
    from types import SimpleNamespace
    from oracle import flowavenet_torch as OT
    rng = np.random.default_rng(B * 1000 + H * 10 + s)
    x = torch.tensor(rng.standard_normal((B, H, W)), requires_grad=True)
    w = torch.tensor(rng.standard_normal((1, 1, 2 * s, 3)) * 0.3, requires_grad=True)
    b = torch.tensor(rng.standard_normal(1), requires_grad=True)
    y = OT.upsample({"upsample_0/w": w, "upsample_0/bias": b}, x, SimpleNamespace(upsample_scales=[s]))     # [B][W][H s]
    y = y.transpose(1, 2).unsqueeze(1)
    assert y.shape == (B, 1, H * s, W)
    dy = rng.standard_normal((B, H * s, W))
    y.backward(torch.tensor(dy).reshape(y.shape))
    ref = ref_upsample_bwd(dy, y.detach().numpy().reshape(B, H * s, W), x.detach().numpy().reshape(B, H, W),
                           w.detach().numpy().reshape(2 * s, 3), s, slope=0.4)
    for got, want in ((ref["dx"], x.grad.numpy().reshape(B, H, W)), (ref["dwk_bias"][:6 * s], w.grad.numpy().reshape(-1)),
                      (ref["dwk_bias"][6 * s:], b.grad.numpy())):
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    # the absolute sums bound their own sums
    assert (np.abs(ref["dx"]) <= ref["dx_abs"] + 1e-15).all() and (np.abs(ref["dwk_bias"]) <= ref["dwk_bias_abs"] + 1e-12).all()


def test_small_gradient_formulas_equal_autograd_through_actnorm_and_zeroconv():
    """db, dlogs and dzscale of include/fwn.h against fp64 autograd of loss = -logdet + <downstream gradient, outputs>
    through ActNorm (y = (x + b) exp(3 logs), logdet += mean_C(3 logs)), the ZeroConv scale ((log_s | t) = Z exp(3 scale))
    and the affine coupling (out_b = (y_b - t) exp(-log_s), logdet += mean(-log_s) / 2) as oracle/flowavenet_torch.py
    defines them (forward(): lines "ActNorm" to "logdet + (-log_s).mean() / 2.0"; restated here, the oracle has them inline).
    Ch = 2, M = 12, both index tables real permutations."""
    Ch, M = 2, 12
    rng = np.random.default_rng(7)
    br, zc = rng.permutation(Ch), rng.permutation(2 * Ch)
    T = lambda a: torch.tensor(a, requires_grad=True)
    b, logs, zscale = T(rng.standard_normal(2 * Ch) * 0.3), T(rng.standard_normal(2 * Ch) * 0.1), T(rng.standard_normal(2 * Ch) * 0.1)
    xa, xb = torch.tensor(rng.standard_normal((M, Ch))), torch.tensor(rng.standard_normal((M, Ch)))
    Z = torch.tensor(rng.standard_normal((M, 2 * Ch)) * 0.3)               # ZeroConv output before its scale factor
    wa, wb = torch.tensor(rng.standard_normal((M, Ch))), torch.tensor(rng.standard_normal((M, Ch)))
    ia, ib, iz = torch.tensor(br), torch.tensor(Ch + br), torch.tensor(zc)
    ya = (xa + b[ia]) * torch.exp(3.0 * logs[ia])
    yb = (xb + b[ib]) * torch.exp(3.0 * logs[ib])
    lt = Z * torch.exp(3.0 * zscale[iz])
    log_s, t = lt[:, :Ch], lt[:, Ch:]
    out_b = (yb - t) * torch.exp(-log_s)
    logdet = (3.0 * logs).mean() + (-log_s).mean() / 2.0
    loss = -logdet + (wa * ya).sum() + (wb * out_b).sum()
    loss.backward()
    # what the kernel is handed at this point of the backward pass (fwn_coupling_bwd's outputs)
    n = lambda v: v.detach().numpy()
    e = np.exp(-n(log_s))
    dls, dt = -n(wb) * n(out_b) + 1.0 / (2.0 * M * Ch), -n(wb) * e
    dzz = np.concatenate([dls * n(log_s), dt * n(t)], 1)
    an = np.zeros((2, 4, Ch))
    for role, idx in enumerate((br, Ch + br)):
        an[role] = [n(b)[idx], np.exp(3.0 * n(logs)[idx]), np.exp(-3.0 * n(logs)[idx]), 3.0 * n(logs)[idx]]
    ref = ref_small_grads(n(wa), n(ya), n(wb) * e, n(yb), dzz, an, br, zc)
    np.testing.assert_allclose(ref["db"], b.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ref["dlogs"], logs.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ref["dzscale"], zscale.grad.numpy(), rtol=1e-12, atol=1e-12)
    # and the in-place half: the planes go back to the flow's input, the gradients to dL/dx
    np.testing.assert_allclose(ref["x0"], n(xa), rtol=0, atol=1e-13)
    np.testing.assert_allclose(ref["x1"], n(xb), rtol=0, atol=1e-13)
    # the constant is really there: without it dlogs is off by exactly 3 / (2 Ch)
    assert np.allclose(ref["dlogs"] + 3.0 / (2.0 * Ch), 3.0 * np.concatenate([(n(wa) * n(ya)).sum(0)[np.argsort(br)],
                                                                            (n(wb) * e * n(yb)).sum(0)[np.argsort(br)]]))
