"""The sum of a seed in front of the norm without a GPU (include/fewbit_hipx.h, "The sum of a seed in front of the norm"; fewbit_amd/csrc/fewbit_norm.hip):
the four fused entry points of the companion library (declared, exported, bound), their refusals before anything is launched, and the fused
functionals and modules on host tensors, where a call IS ``*_norm_quantized(dropout_add(...))``: the same bytes, the same draws."""
import re
import subprocess
from pathlib import Path

import pytest
import torch

import fewbit_amd as fewbit
from fewbit_amd import cabi_x

ROOT = Path(__file__).resolve().parents[1]
ADD_SYMBOLS = ('fewbit_hipx_add_layer_norm_forward', 'fewbit_hipx_add_layer_norm_backward', 'fewbit_hipx_add_rms_norm_forward',
               'fewbit_hipx_add_rms_norm_backward')
DTYPES = (torch.float32, torch.bfloat16, torch.float64)
ids = lambda d: str(d).split('.')[-1] if isinstance(d, torch.dtype) else None
F = fewbit.functional
KINDS = {'layer': (F.dropout_add_layer_norm_quantized, F.layer_norm_quantized, fewbit.DropoutAddLayerNorm, True),
         'rms': (F.dropout_add_rms_norm_quantized, F.rms_norm_quantized, fewbit.DropoutAddRMSNorm, False)}


# ---- the library ------------------------------------------------------------------------------------------------------------------------
def test_the_four_symbols_are_exported_declared_and_bound_and_the_revision_stays():
    header = (ROOT / 'include' / 'fewbit_hipx.h').read_text()
    declared = set(re.findall(r'\b(fewbit_hipx_\w+)\s*\(', header))
    out = subprocess.run(['nm', '-D', '--defined-only', str(cabi_x.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ADD_SYMBOLS:
        assert name in declared and name in exported and name in cabi_x.SYMBOLS, name
    assert declared == set(cabi_x.SYMBOLS) == {name for name in exported if name.startswith('fewbit_hipx_')}
    assert cabi_x.lib().fewbit_hipx_revision() == cabi_x.REVISION == 2 and cabi_x.lib().fewbit_hipx_abi_version() == cabi_x.ABI_VERSION == 1
    assert '#define FEWBIT_HIPX_REVISION 2' in header and 'The sum of a seed in front of the norm' in header
    assert {name[len('fewbit_hipx_'):] for name in ADD_SYMBOLS} <= set(cabi_x.__all__)


def test_calls_are_refused_by_code_and_text_before_anything_is_launched():
    """(null and fake pointers throughout: a call that got as far as a launch would fail loudly)"""
    L = cabi_x.lib()
    err = lambda: L.fewbit_hipx_last_error().decode()
    fake = 4096                                                       # an aligned non-null address that is never dereferenced
    for kind in ('layer', 'rms'):
        fwd, bwd = getattr(L, f'fewbit_hipx_add_{kind}_norm_forward'), getattr(L, f'fewbit_hipx_add_{kind}_norm_backward')
        centred = kind == 'layer'
        ok_f = dict(dtype=2, x=fake, residual=fake, rows=4, width=64, gamma=fake, beta=fake, eps=1e-5, bits=4, seed=1, word=None, threshold=6554, y=fake,
                    h=fake, rstd=fake, state=fake, size=2048, xhat=None, stream=None)
        ok_b = dict(dtype=2, gy=fake, gh=fake, state=fake, rstd=fake, gamma=fake, rows=4, width=64, bits=4, seed=1, word=None, threshold=6554, dres=fake,
                    dbranch=fake, dgamma=fake, dbeta=fake, ws=fake, size=2**20, stream=None)
        if not centred:
            del ok_f['beta'], ok_b['dbeta']
        f = lambda **kw: fwd(*{**ok_f, **kw}.values())
        b = lambda **kw: bwd(*{**ok_b, **kw}.values())
        refused = lambda rc, *words: rc == -1 and all(w in err() for w in words)
        fname, bname = f'add_{kind}_norm_forward', f'add_{kind}_norm_backward'
        # what the plain pair refuses
        assert refused(f(dtype=3), fname, 'dtype 3') and refused(b(dtype=5), bname, 'dtype 5')
        for bits in (0, 3, 16):
            assert refused(f(bits=bits), fname, f'bits = {bits}') and refused(b(bits=bits), bname, f'bits = {bits}')
        for width in (0, 8193):
            assert refused(f(width=width), fname, f'width = {width}') and refused(b(width=width), bname, f'width = {width}')
        assert refused(f(x=None), fname, 'null') and refused(f(y=None), 'null') and refused(f(rstd=None), 'null') and refused(f(residual=None), 'null', 'residual')
        assert refused(b(gy=None), bname, 'null') and refused(b(state=None), 'null') and refused(b(rstd=None), 'null')
        assert refused(b(rstd=None, dres=None), 'null')              # dbranch alone needs rstd too
        for name in ('x', 'residual', 'y', 'h', 'gamma'):
            assert refused(f(**{name: fake + 1}), fname, 'element size'), name
            assert refused(f(dtype=0, **{name: fake + 2}), 'element size'), name
        for name in ('gy', 'gh', 'dres', 'dbranch', 'gamma'):
            assert refused(b(**{name: fake + 1}), bname, 'element size'), name
        assert refused(f(rstd=fake + 2), '4-byte') and refused(b(rstd=fake + 2), '4-byte') and refused(b(dgamma=fake + 2), '4-byte')
        assert refused(f(state=fake + 4), fname, '8-byte') and refused(b(state=fake + 4), bname, '8-byte')
        need = cabi_x.norm_state_bytes(4, 64, 4)
        assert refused(f(size=need - 1), fname, f'{need - 1} bytes, {need} are needed')
        assert refused(f(word=fake + 4), fname, 'seed word') and refused(b(word=fake + 4), bname, 'seed word')
        assert refused(f(eps=-1.0), fname, 'eps')
        assert refused(b(ws=None), bname, 'workspace')
        # what the fusion refuses on top
        for threshold in (65536, 70000):
            assert refused(f(threshold=threshold), fname, f'threshold = {threshold}') and refused(b(threshold=threshold), bname, f'threshold = {threshold}')
        assert f(width=770, size=2**20) == -2 and fname in err() and 'multiple of 8' in err() and '770' in err()      # FEWBIT_ERR_UNSUPPORTED
        assert b(width=770) == -2 and bname in err() and 'multiple of 8' in err()
        assert refused(b(threshold=0), bname, 'dbranch')
        # no rows, and a backward with no output: nothing to do, whatever the pointers
        assert f(rows=0, x=None, y=None) == 0 and b(rows=0, gy=None, state=None) == 0
        assert b(dres=None, dbranch=None, dgamma=None, ws=None, size=0, **({'dbeta': None} if centred else {})) == 0


def test_the_binding_refuses_host_tensors():
    x = torch.zeros(2, 8)
    with pytest.raises(cabi_x.FewbitHipError, match='GPU'):
        cabi_x.add_layer_norm_forward(x, x, None, None, 1e-5)
    with pytest.raises(cabi_x.FewbitHipError, match='GPU'):
        cabi_x.add_rms_norm_backward(x, torch.zeros(64, dtype=torch.uint8), torch.zeros(2), None, 4)


# ---- the functionals and modules on host tensors: the composition ----------------------------------------------------------------------------
def _problem(dtype, width, centred, seed=5):
    g = torch.Generator().manual_seed(seed)
    shape = (3, 4, width)
    x = torch.randn(shape, generator=g).to(dtype).requires_grad_()
    res = (3 + 2 * torch.randn(shape, generator=g)).to(dtype).requires_grad_()
    parameters = ((1 + 0.5 * torch.randn(width, generator=g)).to(dtype).requires_grad_(), )
    if centred:
        parameters += (torch.randn(width, generator=g).to(dtype).requires_grad_(), )
    return x, res, parameters, torch.randn(shape, generator=g).to(dtype), torch.randn(shape, generator=g).to(dtype)


@pytest.mark.parametrize('prenorm', (False, True))
@pytest.mark.parametrize('dtype', DTYPES, ids=ids)
@pytest.mark.parametrize('kind', KINDS)
def test_on_host_tensors_the_call_is_the_composition(kind, dtype, prenorm):
    fused, norm, _, centred = KINDS[kind]
    for width, p in ((64, 0.25), (9, 0.5), (70, 0.0)):
        x, res, parameters, gy, gh = _problem(dtype, width, centred)
        leaves = (x, res, *parameters)

        def gradients(y, h):
            outs, grads = ((y, h), (gy, gh)) if prenorm else ((y, ), (gy, ))
            return torch.autograd.grad(outs, leaves, grads)

        torch.manual_seed(21)
        h0 = F.dropout_add(x, res, p, True)
        y0 = norm(h0, (width, ), *parameters, 1e-5, 4)
        want, state = gradients(y0, h0), torch.get_rng_state()
        torch.manual_seed(21)
        out = fused(x, res, (width, ), *parameters, 1e-5, p, True, 4, prenorm)
        y, h = out if prenorm else (out, None)
        assert isinstance(out, tuple) == prenorm
        assert torch.equal(y, y0) and (h is None or torch.equal(h, h0))
        got = gradients(y, h if prenorm else None)
        assert torch.equal(torch.get_rng_state(), state)
        assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize('kind', KINDS)
def test_the_modules_share_parameters_follow_eval_and_say_what_they_are(kind):
    fused, norm, module, centred = KINDS[kind]
    width = 24
    base = torch.nn.LayerNorm(width, eps=1e-6) if centred else torch.nn.RMSNorm(width, eps=1e-6)
    layer = (module.from_layer_norm if centred else module.from_rms_norm)(base, p=0.5, prenorm=True, bits=2)
    assert isinstance(layer, fewbit.QuantizedLayerNorm if centred else fewbit.QuantizedRMSNorm) and layer.weight is base.weight
    assert (layer.p, layer.prenorm, layer.bits, layer.eps) == (0.5, True, 2, 1e-6) and 'p=0.5, prenorm=True' in repr(layer) and 'bits=2' in repr(layer)
    x, res, _, gy, gh = _problem(torch.float32, width, centred)
    parameters = (layer.weight, layer.bias) if centred else (layer.weight, )
    torch.manual_seed(4)
    y, h = layer(x, res)
    torch.manual_seed(4)
    y0, h0 = fused(x, res, (width, ), *parameters, 1e-6, 0.5, True, 2, True)
    assert torch.equal(y, y0) and torch.equal(h, h0) and not torch.equal(h, res + x)
    # eval: no dropout, and the gradients are torch's exact ones on residual + input
    layer.eval()
    y, h = layer(x, res)
    assert torch.equal(h, res + x) and torch.equal(y, base(res + x)) and 'Quantized' not in type(y.grad_fn).__name__
    with torch.no_grad():
        y2, h2 = layer(x, res)
    assert torch.equal(y2, y) and torch.equal(h2, h) and y2.grad_fn is None
    plain = module(width, p=0.1)
    assert plain.prenorm is False and plain.p == 0.1 and not isinstance(plain.train()(x.detach(), res.detach()), tuple)


@pytest.mark.parametrize('kind', KINDS)
def test_refusals_are_worded_like_the_existing_ones(kind):
    fused, _, module, _ = KINDS[kind]
    x = torch.zeros(2, 8)
    for bits in (0, 3, 16):
        with pytest.raises(ValueError, match=f'bits should be 2, 4 or 8, but got {bits}.'):
            fused(x, x, (8, ), bits=bits)
        with pytest.raises(ValueError, match=f'bits should be 2, 4 or 8, but got {bits}.'):
            module(8, bits=bits)
    for p in (-0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match='dropout probability has to be between 0 and 1, but got'):
            fused(x, x, (8, ), p=p)
        with pytest.raises(ValueError, match='dropout probability has to be between 0 and 1, but got'):
            module(8, p=p)
    with pytest.raises(ValueError, match=r'residual should have the shape of input, \(2, 8\), but got \(8,\)'):
        fused(x, torch.zeros(8), (8, ))
