"""``fewbit.MXMLP`` / ``fewbit.functional.mlp_mx`` on host tensors (fewbit_amd/mlp.py), the composed route: fp32, 96 tokens, 64 -> 96 -> 64.  The output is
torch's MLP bit for bit; the four gradients are the documented formulas evaluated here from ``mx_pack_host`` / ``mx_unpack_host`` with the seeds of
``MLP_MX_SEEDS`` (the call's one draw plus 0 .. 3; nothing is rounded to fp8 on this route), to the summation order of fp32: at most 1e-5 of the largest
entry.  That pins the seed order, the roles and the formulas.  No GPU needed."""
import pytest
import torch
import torch.nn.functional as F

import fewbit
from fewbit_amd import cabi_x, linear

ACTS = {'gelu': F.gelu, 'gelu_tanh': lambda t: F.gelu(t, approximate='tanh'), 'relu': F.relu, 'silu': F.silu}


@pytest.mark.parametrize('format', ('fp4', 'fp6'))
@pytest.mark.parametrize('activation', tuple(ACTS))
def test_the_output_is_torchs_and_the_gradients_are_the_formulas_on_the_decodes(activation, format):
    torch.manual_seed(3)
    mlp = fewbit.MXMLP(64, 96, activation=activation, format=format, generator=torch.Generator().manual_seed(11))
    assert fewbit.MXMLP is fewbit.mlp.MXMLP and fewbit.functional.mlp_mx is fewbit.mlp.mlp_mx and fewbit.mlp.MLP_MX_SEEDS == ('x', 'u', 'd_u', 'product', 'grad_output')
    x, G = torch.randn(96, 64, requires_grad=True), torch.randn(96, 64)
    (W1, b1), (W2, b2) = ((layer.weight, layer.bias) for layer in (mlp.fc1, mlp.fc2))
    out = mlp(x)
    assert out.grad_fn.name() == '_MLPMXBackward' and torch.equal(out, F.linear(ACTS[activation](F.linear(x, W1, b1)), W2, b2))
    got = torch.autograd.grad(out, (x, W1, b1, W2), G)
    base = linear._draw_seed(torch.Generator().manual_seed(11))
    rounded = lambda t, i: cabi_x.mx_unpack_host(cabi_x.mx_pack_host(t, base + i, format, 'kept'), *t.shape, format)
    with torch.no_grad():
        x_hat, u_hat = rounded(x, 0), rounded(F.linear(x, W1, b1), 1)
    u64 = u_hat.double().requires_grad_()
    slope = torch.autograd.grad(ACTS[activation](u64).sum(), u64)[0].float()
    with torch.no_grad():
        du = (G @ W2) * slope
        want = (du @ W1, du.T @ x_hat, du.sum(dim=0), G.T @ rounded(ACTS[activation](u_hat), 3))
    for name, a, b in zip(('dx', 'dW1', 'db1', 'dW2'), got, want):
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()), name


def test_unknown_choices_are_refused_by_name():
    x, W = torch.randn(4, 64), torch.randn(64, 64)
    with pytest.raises(ValueError, match="'gelu', 'gelu_tanh', 'relu', 'silu'"):
        fewbit.functional.mlp_mx(x, W, W, activation='tanh')
    with pytest.raises(ValueError, match="'fp4' or 'fp6'"):
        fewbit.MXMLP(64, 64, format='fp8')
