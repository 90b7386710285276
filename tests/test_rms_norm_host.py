"""The un-centred rows without a GPU (include/fewbit_hipx.h, "The un-centred rows"; fewbit_amd/csrc/fewbit_norm.hip): the two RMS-norm entry points
of the companion library (declared, exported, bound), their refusals before anything is launched, and ``fewbit.QuantizedRMSNorm`` on host
tensors: the forward value, what is saved, the gradients on the saved codes, ``eps=None``, ``from_rms_norm``, and the statistics of the
definition over 200 calls (the two statistics and thresholds of tests/test_norm_host.py)."""
import math
import re
import subprocess
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import fewbit_amd as fewbit
from fewbit_amd import cabi, cabi_x, norm
from norm_harness import RMS_NORM as KIND, input_gradient_averages_out, saved_by, weight_gradient_is_unbiased

ROOT = Path(__file__).resolve().parents[1]
RMS_SYMBOLS = ('fewbit_hipx_rms_norm_forward', 'fewbit_hipx_rms_norm_backward')
BITS = (2, 4, 8)
WIDTHS = (1, 7, 8, 9, 63, 64, 65, 200, 770)
DTYPES = (torch.float32, torch.bfloat16, torch.float64)
ids = lambda d: str(d).split('.')[-1] if isinstance(d, torch.dtype) else None


# ---- the library ------------------------------------------------------------------------------------------------------------------------
def test_the_two_symbols_are_exported_declared_and_bound_and_the_revision_stays():
    header = (ROOT / 'include' / 'fewbit_hipx.h').read_text()
    declared = set(re.findall(r'\b(fewbit_hipx_\w+)\s*\(', header))
    out = subprocess.run(['nm', '-D', '--defined-only', str(cabi_x.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in RMS_SYMBOLS:
        assert name in declared and name in exported and name in cabi_x.SYMBOLS, name
    assert declared == set(cabi_x.SYMBOLS) == {name for name in exported if name.startswith('fewbit_hipx_')}
    assert cabi_x.lib().fewbit_hipx_revision() == cabi_x.REVISION == 2 and cabi_x.lib().fewbit_hipx_abi_version() == cabi_x.ABI_VERSION == 1
    assert '#define FEWBIT_HIPX_REVISION 2' in header and 'The un-centred rows' in header
    assert {'rms_norm_forward', 'rms_norm_backward'} <= set(cabi_x.__all__)


def test_calls_are_refused_by_code_and_text_before_anything_is_launched():
    """(null and fake pointers throughout: a call that got as far as a launch would fail loudly)"""
    L = cabi_x.lib()
    err = lambda: L.fewbit_hipx_last_error().decode()
    fwd, bwd = L.fewbit_hipx_rms_norm_forward, L.fewbit_hipx_rms_norm_backward
    fake = 4096                                                       # an aligned non-null address that is never dereferenced
    ok_f = dict(dtype=2, x=fake, rows=4, width=64, gamma=fake, eps=1e-5, bits=4, seed=1, word=None, y=fake, rstd=fake, state=fake, size=2048, xhat=None,
                stream=None)
    ok_b = dict(dtype=2, gy=fake, state=fake, rstd=fake, gamma=fake, rows=4, width=64, bits=4, dx=fake, dgamma=fake, ws=fake, size=2**20, stream=None)
    f = lambda **kw: fwd(*{**ok_f, **kw}.values())
    b = lambda **kw: bwd(*{**ok_b, **kw}.values())
    refused = lambda rc, *words: rc == -1 and all(w in err() for w in words)
    assert refused(f(dtype=3), 'rms_norm_forward', 'dtype 3') and refused(b(dtype=5), 'rms_norm_backward', 'dtype 5')
    for bits in (0, 1, 3, 5, 16):
        assert refused(f(bits=bits), 'rms_norm_forward', f'bits = {bits}') and refused(b(bits=bits), 'rms_norm_backward', f'bits = {bits}')
    for width in (0, 8193):
        assert refused(f(width=width), 'rms_norm_forward', f'width = {width}') and refused(b(width=width), 'rms_norm_backward', f'width = {width}')
    assert refused(f(rows=2**36 // 64 + 1, size=2**40), 'rms_norm_forward', '2^36') and refused(b(rows=2**36 // 64 + 1), 'rms_norm_backward', '2^36')
    assert refused(f(x=None), 'rms_norm_forward', 'null') and refused(f(y=None), 'null') and refused(f(rstd=None), 'null')
    assert refused(b(gy=None), 'rms_norm_backward', 'null') and refused(b(state=None), 'null') and refused(b(rstd=None), 'null')
    for name in ('x', 'y', 'gamma'):
        assert refused(f(**{name: fake + 1}), 'rms_norm_forward', 'element size'), name
        assert refused(f(dtype=0, **{name: fake + 2}), 'element size'), name
    for name in ('gy', 'dx', 'gamma'):
        assert refused(b(**{name: fake + 1}), 'rms_norm_backward', 'element size'), name
    assert 'beta' not in err()
    assert refused(f(rstd=fake + 2), '4-byte') and refused(f(xhat=fake + 2), '4-byte')
    assert refused(b(rstd=fake + 2), '4-byte') and refused(b(dgamma=fake + 2), '4-byte') and 'dbeta' not in err()
    assert refused(f(state=fake + 4), 'rms_norm_forward', '8-byte') and refused(b(state=fake + 4), 'rms_norm_backward', '8-byte')
    need = cabi_x.norm_state_bytes(4, 64, 4)
    assert refused(f(size=need - 1), 'rms_norm_forward', f'{need - 1} bytes, {need} are needed')
    assert refused(f(word=fake + 4), 'seed word')
    assert refused(f(eps=-1.0), 'rms_norm_forward', 'eps') and refused(f(eps=float('nan')), 'eps') and refused(f(eps=float('inf')), 'eps')
    assert refused(b(ws=None), 'rms_norm_backward', 'workspace') and refused(b(ws=fake + 8), 'workspace')
    need = cabi_x.norm_workspace_bytes(4, 64)
    assert refused(b(size=need - 1), 'rms_norm_backward', f'{need - 1} bytes, {need} are needed')
    # no rows, and a backward with no output: nothing to do, whatever the pointers
    assert f(rows=0, x=None, y=None) == 0 and b(rows=0, gy=None, state=None) == 0 and b(dx=None, dgamma=None, ws=None, size=0) == 0
    # the plain forward ignores bits
    assert refused(f(state=None, bits=3, x=None), 'null')


def test_the_binding_refuses_host_tensors():
    with pytest.raises(cabi.FewbitHipError, match='GPU'):
        cabi_x.rms_norm_forward(torch.zeros(2, 8), None, 1e-5)
    with pytest.raises(cabi.FewbitHipError, match='GPU'):
        cabi_x.rms_norm_backward(torch.zeros(2, 8), torch.zeros(64, dtype=torch.uint8), torch.zeros(2), None, 4)


# ---- fewbit.QuantizedRMSNorm on the host ---------------------------------------------------------------------------------------------------
formula64, exact_rows = KIND.formula64, KIND.exact_rows          # (dx, dgamma) and (x^, rstd) of the definition in float64


@pytest.mark.parametrize('bits', BITS)
@pytest.mark.parametrize('dtype', DTYPES, ids=ids)
def test_layer_on_host_tensors(dtype, bits):
    work = torch.float64 if dtype == torch.float64 else torch.float32         # the dtype of what the formulation keeps
    for width in WIDTHS:
        torch.manual_seed(3 + width)
        rows, eps = 12, 1e-6
        layer = fewbit.QuantizedRMSNorm(width, eps=eps, dtype=dtype, bits=bits)
        with torch.no_grad():
            layer.weight.copy_(torch.randn(width) + 1)
        x = (3 + 2 * torch.randn(3, rows // 3, width)).to(dtype).requires_grad_()  # (three dimensions: the rows are the leading two)
        gy = torch.randn(3, rows // 3, width).to(dtype)
        y, saved = saved_by(lambda: layer(x))
        assert type(y.grad_fn).__name__ == '_RMSNormQuantizedBackward' and y.dtype == dtype
        assert torch.equal(y, F.rms_norm(x, (width, ), layer.weight, eps))
        # exactly codes (one per byte of the padded rows), lo, step, rstd and gamma: never the input
        groups = math.ceil(width / 64)
        assert [(t.dtype, t.numel()) for t in saved] == [(torch.uint8, rows * groups * 64), (work, rows * groups), (work, rows * groups), (work, rows), (dtype, width)]
        assert saved[4] is layer.weight or saved[4].data_ptr() == layer.weight.data_ptr()
        assert all(t.data_ptr() != x.data_ptr() for t in saved)
        codes, lo, step, rstd, gamma = saved
        assert int(codes.max()) <= 2**bits - 1
        xq = torch.addcmul(lo.double()[:, None], codes.view(-1, 64).double(), step.double()[:, None]).view(rows, -1)[:, :width]
        xhat, rstd64 = exact_rows(x.detach().reshape(rows, width), eps)
        assert bool(((xq - xhat).abs() <= step.double().view(rows, groups).repeat_interleave(64, dim=1)[:, :width] * (1 + 1e-6) + 1e-5).all())
        assert bool(((rstd.double() - rstd64).abs() <= (1e-12 if dtype == torch.float64 else 1e-6) * rstd64).all())
        gx, gw = torch.autograd.grad(y, (x, layer.weight), gy)
        assert gx.shape == x.shape and gx.dtype == gw.dtype == dtype and gw.shape == (width, )
        # the gradients are the formula on the saved codes: float64 arithmetic to 1e-12, fp32 arithmetic to its own rounding, then the dtype's
        dx, dgamma = formula64(gy.reshape(rows, width), xq, rstd, gamma)
        unit = {torch.float64: 1e-12, torch.float32: 1e-5, torch.bfloat16: 2.0**-8 + 1e-5}[dtype]
        scale_x = rstd.double()[:, None] * ((gy.double().reshape(rows, width) * gamma.double()).abs() + xq.abs() * (gy.double().reshape(rows, width) * gamma.double() * xq).abs().mean(dim=1, keepdim=True))
        assert bool(((gx.double().reshape(rows, width) - dx).abs() <= unit * scale_x.clamp_min(1e-30)).all()), width
        assert bool(((gw.double() - dgamma).abs() <= unit * (gy.double().reshape(rows, width) * xq).abs().sum(dim=0).clamp_min(1e-30)).all()), width


@pytest.mark.parametrize('dtype', DTYPES, ids=ids)
def test_eps_none_resolves_per_dtype_and_no_weight_works(dtype):
    x = (1 + torch.randn(6, 70)).to(dtype).requires_grad_()
    layer = fewbit.QuantizedRMSNorm(70, dtype=dtype, elementwise_affine=False)
    assert layer.eps is None and layer.weight is None
    y, saved = saved_by(lambda: layer(x))
    # torch.finfo(input.dtype).eps, the default torch documents.  (For a 16-bit HOST tensor torch 2.10's own F.rms_norm(eps=None) takes the epsilon of
    # its fp32 arithmetic type instead, so there the comparison is with the documented value passed explicitly.)
    assert torch.equal(y, F.rms_norm(x, (70, ), None, torch.finfo(dtype).eps)) and (dtype == torch.bfloat16 or torch.equal(y, F.rms_norm(x, (70, ))))
    assert len(saved) == 4 and saved[0].dtype == torch.uint8                       # codes, lo, step, rstd: no weight
    _, rstd64 = exact_rows(x.detach(), torch.finfo(dtype).eps)
    assert bool(((saved[3].double() - rstd64).abs() <= 1e-6 * rstd64).all())
    # at a tiny row eps decides rstd, so a wrong default would show: bf16's eps is 2^-7, fp32's 2^-23
    tiny = torch.full((1, 8), 1e-3).to(dtype).requires_grad_()
    _, saved = saved_by(lambda: fewbit.functional.rms_norm_quantized(tiny, (8, )))
    want = 1.0 / math.sqrt(float(tiny.detach().double().square().mean()) + torch.finfo(dtype).eps)
    assert abs(float(saved[3]) - want) <= 1e-6 * want
    (gx, ) = torch.autograd.grad(y, x, torch.randn(6, 70).to(dtype))
    assert gx.shape == x.shape and gx.dtype == dtype


def test_layer_arguments_repr_and_exports():
    for bits in (0, 1, 3, 5, 16):
        with pytest.raises(ValueError, match='bits should be 2, 4 or 8'):
            fewbit.QuantizedRMSNorm(4, bits=bits)
        with pytest.raises(ValueError, match='bits should be 2, 4 or 8'):
            fewbit.functional.rms_norm_quantized(torch.zeros(2, 4), (4, ), bits=bits)
    m = fewbit.QuantizedRMSNorm(6, eps=1e-6, bits=8)
    assert isinstance(m, torch.nn.RMSNorm) and repr(m) == 'QuantizedRMSNorm((6,), eps=1e-06, elementwise_affine=True, bits=8)'
    assert fewbit.QuantizedRMSNorm(6).bits == 4 and fewbit.QuantizedRMSNorm(6).generator is None
    assert fewbit.QuantizedRMSNorm is norm.QuantizedRMSNorm and fewbit.functional.rms_norm_quantized is norm.rms_norm_quantized
    import fewbit as alias
    assert alias.QuantizedRMSNorm is norm.QuantizedRMSNorm and alias.functional.rms_norm_quantized is norm.rms_norm_quantized
    assert {'QuantizedRMSNorm', 'rms_norm_quantized'} <= set(norm.__all__)
    assert 'QuantizedRMSNorm' not in fewbit.modules.__all__ and 'rms_norm_quantized' not in fewbit.modules.__all__
    with pytest.raises(RuntimeError, match='normalized_shape'):                   # a shape mismatch is left to torch's wording
        fewbit.functional.rms_norm_quantized(torch.zeros(2, 6), (5, ))
    # a normalized shape of two dimensions, an int for one
    x = torch.randn(3, 5, 6, requires_grad=True)
    y, saved = saved_by(lambda: fewbit.functional.rms_norm_quantized(x, (5, 6), bits=4))
    assert torch.equal(y, F.rms_norm(x, (5, 6))) and len(saved) == 4 and saved[0].numel() == 3 * 64
    (gx, ) = torch.autograd.grad(y, x, torch.randn(3, 5, 6))
    assert gx.shape == x.shape
    assert torch.equal(fewbit.functional.rms_norm_quantized(x, 6, eps=1e-6), F.rms_norm(x, (6, ), None, 1e-6))


class StandInRMSNorm(torch.nn.Module):
    """the shape of LlamaRMSNorm / T5LayerNorm: a 1-D weight, `variance_epsilon`, x^ rounded to the input's dtype before the weight"""

    def __init__(self, hidden, eps=1e-6):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(hidden))
        self.variance_epsilon = eps

    def forward(self, hidden_states):
        dtype = hidden_states.dtype
        h = hidden_states.to(torch.float32)
        h = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + self.variance_epsilon)
        return self.weight * h.to(dtype)


def test_from_rms_norm_shares_the_weight_and_map_module_swaps_a_model():
    model = torch.nn.Sequential(torch.nn.RMSNorm(4, eps=1e-5), torch.nn.Linear(4, 8), torch.nn.Sequential(torch.nn.RMSNorm(8, elementwise_affine=False)),
                                StandInRMSNorm(8, 1e-6), fewbit.QuantizedRMSNorm(8, bits=8)).eval()
    with torch.no_grad():
        model[0].weight.copy_(torch.randn(4) + 1)
        model[3].weight.copy_(torch.randn(8) + 1)
    weight, stand_in_weight = model[0].weight, model[3].weight
    x = torch.randn(5, 4)
    before = model(x)

    def swap(m, path):
        return fewbit.QuantizedRMSNorm.from_rms_norm(m, bits=2) if type(m) in (torch.nn.RMSNorm, StandInRMSNorm) else m

    model = fewbit.map_module(model, swap)
    swapped = [m for m in model.modules() if type(m) is fewbit.QuantizedRMSNorm]
    assert [m.bits for m in swapped] == [2, 2, 2, 8] and swapped[0].weight is weight and swapped[1].weight is None and swapped[2].weight is stand_in_weight
    assert not swapped[0].training and swapped[0].eps == 1e-5 and swapped[0].normalized_shape == (4, )
    assert swapped[1].eps is None and swapped[2].eps == 1e-6 and swapped[2].normalized_shape == (8, ) and not swapped[2].training
    assert not any(p.is_meta for p in model.parameters())
    assert bool(((model(x) - before).abs() <= 1e-5 * before.abs().clamp_min(1.0)).all())          # fp32: the stand-in and F.rms_norm agree to rounding
    model.train()
    xg = torch.randn(5, 4, requires_grad=True)
    y = model(xg)
    assert y.shape == (5, 8) and type(y.grad_fn).__name__ == '_RMSNormQuantizedBackward'
    y.sum().backward()
    assert weight.grad is not None and stand_in_weight.grad is not None and xg.grad.shape == xg.shape
    # the `eps` spelling, and what is not a norm
    other = torch.nn.Module()
    other.weight, other.eps = torch.nn.Parameter(torch.ones(3)), 1e-6
    assert fewbit.QuantizedRMSNorm.from_rms_norm(other).weight is other.weight
    with pytest.raises(TypeError, match='1-D weight'):
        fewbit.QuantizedRMSNorm.from_rms_norm(torch.nn.Linear(3, 3))


def test_no_grad_and_nothing_that_requires_grad_keep_nothing_and_draw_nothing():
    layer = fewbit.QuantizedRMSNorm(24, eps=1e-6)
    x = torch.randn(12, 24, requires_grad=True)
    state = torch.get_rng_state()
    with torch.no_grad():
        y, saved = saved_by(lambda: layer(x))
    assert y.grad_fn is None and not saved and torch.equal(y, F.rms_norm(x, (24, ), layer.weight, 1e-6))
    layer.requires_grad_(False)
    y, saved = saved_by(lambda: layer(x.detach()))
    assert y.grad_fn is None and not saved
    y, saved = saved_by(lambda: layer.eval()(x.detach()))
    assert y.grad_fn is None and not saved
    y, saved = saved_by(lambda: layer.eval()(x))                     # eval with gradients: torch's exact RMS norm, no codes, no seed
    assert 'Quantized' not in type(y.grad_fn).__name__ and not any(t.dtype == torch.uint8 for t in saved)
    (gx, ) = torch.autograd.grad(y, x, torch.ones_like(y))
    x2 = x.detach().clone().requires_grad_()
    (want, ) = torch.autograd.grad(F.rms_norm(x2, (24, ), layer.weight, 1e-6), x2, torch.ones_like(y))
    assert torch.equal(gx, want)
    assert torch.equal(torch.get_rng_state(), state)                 # and nothing was drawn


def test_the_generator_decides_the_rounding_and_checkpointing_reproduces_it():
    from torch.utils.checkpoint import checkpoint
    x, w = torch.randn(12, 70, requires_grad=True), torch.randn(70, requires_grad=True)
    gy = torch.randn(12, 70)

    def grads(generator=None):
        return torch.autograd.grad(fewbit.functional.rms_norm_quantized(x, (70, ), w, 1e-5, 2, generator), (x, w), gy)

    a, c = grads(torch.Generator().manual_seed(4)), grads(torch.Generator().manual_seed(4))
    assert all(torch.equal(p, q) for p, q in zip(a, c)) and not torch.equal(a[1], grads(torch.Generator().manual_seed(5))[1])
    torch.manual_seed(8)
    plain = grads()
    for reentrant in (False, True):
        torch.manual_seed(8)
        y = checkpoint(lambda t, weight: fewbit.functional.rms_norm_quantized(t, (70, ), weight, 1e-5, 2), x, w, use_reentrant=reentrant)
        x.grad = w.grad = None
        y.backward(gy)
        assert all(torch.equal(p.grad, q) for p, q in zip((x, w), plain)), reentrant
    x.grad = w.grad = None


# ---- the statistics of the definition: 200 calls, fp32 host tensors, seeds from torch.manual_seed(0) (norm_harness) ------------------------------
@pytest.mark.parametrize('bits', BITS)
@pytest.mark.parametrize('shape', ((48, 200), (32, 64), (40, 8)), ids=lambda s: 'x'.join(map(str, s)))
def test_the_weight_gradient_is_unbiased(shape, bits):
    weight_gradient_is_unbiased(KIND, shape, bits)


@pytest.mark.parametrize('bits', BITS)
@pytest.mark.parametrize('shape', ((48, 200), (24, 770)), ids=lambda s: 'x'.join(map(str, s)))
def test_the_input_gradient_averages_out_up_to_its_second_order_bias(shape, bits):
    input_gradient_averages_out(KIND, shape, bits)
