"""``fewbit.DropoutAddLayerNorm`` / ``DropoutAddRMSNorm`` and their functionals on the GPU: ONE node that draws ONE seed, keeps what the plain
quantized norm keeps (the state, ``rstd``, gamma -- nothing of the input's size) and gives, bit for bit, the output and every gradient of the
composition run BY HAND with that one seed: ``cabi_x.dropout_apply`` then the plain norm's entry points, then torch's add of the gradient
arriving at ``h`` and the dropout's own backward.  Inside training wrappers the shared bodies of tests/norm_harness.py run on a ``Kind`` that binds
the residual (and, where a body compares with the entry points, composes them as above)."""
import pytest
import torch
import torch.nn.functional as F

import fewbit
import norm_harness as harness
from fewbit_amd import cabi_x
from norm_harness import DEV, EPS, native_sketch_on, saved_by, seeds  # noqa: F401 (the fixtures are used by name)

pytestmark = pytest.mark.gpu
KINDS = {'layer': (harness.LAYER_NORM, fewbit.functional.dropout_add_layer_norm_quantized, fewbit.DropoutAddLayerNorm),
         'rms': (harness.RMS_NORM, fewbit.functional.dropout_add_rms_norm_quantized, fewbit.DropoutAddRMSNorm)}
SHAPES = ((2, 37, 768), (5, 7, 4104))
ids = lambda d: str(d).split('.')[-1] if isinstance(d, torch.dtype) else None


def residual_of(shape, dtype, requires_grad=True):
    g = torch.Generator().manual_seed(977)
    return (3 + 2 * torch.randn(*shape, generator=g)).to(dtype).to(DEV).requires_grad_(requires_grad)


def composed(plain, x, res, parameters, gy, gh, bits, seed, p):
    """(y, h, (dbranch, dres, dgamma[, dbeta]), state, rstd) of the existing calls with ONE seed, as tests/test_gpu_add_norm.py composes them"""
    width = x.shape[-1]
    flat, r = x.detach().reshape(-1, width).contiguous(), res.detach().reshape(-1, width).contiguous()
    mask = cabi_x.dropout_threshold(p) > 0
    h = cabi_x.dropout_apply(flat, seed, p, addend=r) if mask else flat + r
    parameters = tuple(t.detach() for t in parameters)
    y, rstd, state, _ = plain.forward(h, *parameters, EPS, bits, seed)
    g = gy.reshape(flat.shape).contiguous()
    dx, *sums = plain.backward(g, state, rstd, parameters[0], bits)
    if gh is None:
        dres = dx
    elif g.dtype == torch.float32:
        dres = dx + gh.reshape(flat.shape)
    else:
        dx32 = plain.backward(g.float(), state, rstd, parameters[0].float(), bits)[0]
        dres = (dx32 + gh.reshape(flat.shape).float()).to(g.dtype)
    dbranch = cabi_x.dropout_apply(dres, seed, p) if mask else dres
    return y.view(x.shape), h.view(x.shape), (dbranch.view(x.shape), dres.view(x.shape), *sums), state, rstd


def bound(name, shape, p):
    """the ``Kind`` of the fused layer with the residual bound, for the shared bodies of the harness: ``functional`` is the fused functional,
    ``forward`` / ``backward`` are the composition of the existing entry points with the seed the forward was given"""
    plain, fused, module = KINDS[name]
    base = residual_of(shape, torch.float32, False)
    res = lambda x: base.to(x.dtype).view(x.shape)
    seen = {}

    def functional(x, normalized_shape, *rest):
        *parameters, eps, bits = rest
        return fused(x, res(x), normalized_shape, *parameters, eps=eps, p=p, bits=bits)

    def forward(flat, *rest):
        *parameters, eps, bits, seed = rest
        seen['seed'] = seed
        h = cabi_x.dropout_apply(flat, seed, p, addend=res(flat).contiguous()) if cabi_x.dropout_threshold(p) else flat + res(flat)
        return plain.forward(h, *parameters, eps, bits, seed)

    def backward(gy, state, rstd, gamma, bits):
        dx, *sums = plain.backward(gy, state, rstd, gamma, bits)
        return (cabi_x.dropout_apply(dx, seen['seed'], p) if cabi_x.dropout_threshold(p) else dx, *sums)

    class Bound(module):

        def forward(self, x):
            return super().forward(x, res(x))

    return harness.Kind(functional, lambda *a, **kw: Bound(*a, p=p, **kw), forward, backward, '_DropoutAddNormQuantizedBackward', plain.centred)


@pytest.mark.parametrize('prenorm', (False, True), ids=('postnorm', 'prenorm'))
@pytest.mark.parametrize('bits', (2, 4, 8))
@pytest.mark.parametrize('dtype', (torch.float32, torch.float16, torch.bfloat16), ids=ids)
@pytest.mark.parametrize('name', KINDS)
def test_one_seed_one_node_the_norms_savings_and_the_compositions_bits(name, dtype, bits, prenorm, seeds):
    plain, fused, _ = KINDS[name]
    for shape, p in zip(SHAPES, (0.1, 0.5)):
        x, parameters, gy = harness.problem(plain, shape, dtype)
        res = residual_of(shape, dtype)
        gh = torch.randn_like(gy) if prenorm else None
        del seeds[:]
        out, saved = saved_by(lambda: fused(x, res, (shape[-1], ), *parameters, eps=EPS, p=p, bits=bits, prenorm=prenorm))
        y, h = out if prenorm else (out, None)
        assert len(seeds) == 1 and type(y.grad_fn).__name__ == '_DropoutAddNormQuantizedBackward' and (h is None or h.grad_fn is y.grad_fn)
        # saved: the state, rstd and gamma, the bytes of the plain quantized norm on this shape -- and no tensor of the input's size
        _, saved_plain = saved_by(lambda: plain.functional(x, (shape[-1], ), *parameters, EPS, bits))
        assert [(t.dtype, t.numel()) for t in saved] == [(t.dtype, t.numel()) for t in saved_plain] and len(saved) == 3
        assert saved[0].dtype == torch.uint8 and saved[1].dtype == torch.float32 and saved[2].data_ptr() == parameters[0].data_ptr()
        assert all(t.numel() * t.element_size() < x.numel() * x.element_size() for t in saved)
        ye, he, grads_e, state, rstd = composed(plain, x, res, parameters, gy, gh, bits, seeds[0], p)
        assert torch.equal(y, ye) and torch.equal(saved[0], state) and torch.equal(saved[1], rstd) and (h is None or torch.equal(h, he))
        # a loss that uses h as well (pre-norm: the residual stream goes on)
        grads = torch.autograd.grad((y, h) if prenorm else (y, ), (x, res, *parameters), (gy, gh) if prenorm else (gy, ))
        assert len(grads) == len(grads_e)
        for got, want, leaf in zip(grads, grads_e, (x, res, *parameters)):
            assert got.dtype == leaf.dtype and torch.equal(got, want.to(leaf.dtype).view(leaf.shape))


@pytest.mark.parametrize('name', KINDS)
def test_frozen_gamma_a_residual_without_grad_and_a_loss_on_h_alone(name, seeds):
    plain, fused, _ = KINDS[name]
    shape, dtype, bits, p = SHAPES[0], torch.bfloat16, 4, 0.1
    x, parameters, gy = harness.problem(plain, shape, dtype, 1)
    res = residual_of(shape, dtype, False)
    parameters[0].requires_grad_(False)
    leaves = (x, *parameters[1:])
    y, h = fused(x, res, (shape[-1], ), *parameters, eps=EPS, p=p, bits=bits, prenorm=True)
    gh = torch.randn_like(gy)
    _, _, (dbranch, _, _, *rest), _, _ = composed(plain, x, res, parameters, gy, gh, bits, seeds[-1], p)
    grads = torch.autograd.grad((y, h), leaves, (gy, gh), retain_graph=True)
    assert torch.equal(grads[0], dbranch) and all(torch.equal(a, b.to(a.dtype)) for a, b in zip(grads[1:], rest))
    # only h reaches the loss: the norm contributes the terms of a zero gradient, the branch gets the dropout's backward of gh
    only_h = torch.autograd.grad(h, x, gh)[0]
    assert torch.equal(only_h, composed(plain, x, res, parameters, torch.zeros_like(gy), gh, bits, seeds[-1], p)[2][0])


@pytest.mark.parametrize('name', KINDS)
def test_without_a_mask_one_tensor_serves_both_gradients_and_no_h_is_written_twice(name, seeds):
    plain, fused, _ = KINDS[name]
    shape, dtype, bits = (3, 5, 770), torch.bfloat16, 4                     # (no mask: any width is on the kernel path)
    x, parameters, gy = harness.problem(plain, shape, dtype, 2)
    res = residual_of(shape, dtype)
    y = fused(x, res, (shape[-1], ), *parameters, eps=EPS, p=0.0, bits=bits)
    assert len(seeds) == 1 and type(y.grad_fn).__name__ == '_DropoutAddNormQuantizedBackward'
    gx, gr, *sums = torch.autograd.grad(y, (x, res, *parameters), gy)
    ye, _, (dbranch, dres, *sums_e), _, _ = composed(plain, x, res, parameters, gy, None, bits, seeds[0], 0.0)
    assert torch.equal(y, ye) and torch.equal(gx, dres) and torch.equal(gr, dres) and gx.data_ptr() == gr.data_ptr()
    assert all(torch.equal(a, b.to(a.dtype)) for a, b in zip(sums, sums_e))


@pytest.mark.parametrize('name', KINDS)
def test_a_mask_at_a_width_that_is_no_multiple_of_8_takes_the_composed_path(name, seeds):
    plain, fused, _ = KINDS[name]
    shape, dtype, bits, p = (3, 5, 770), torch.bfloat16, 4, 0.1
    x, parameters, gy = harness.problem(plain, shape, dtype, 3)
    res = residual_of(shape, dtype)
    leaves = (x, res, *parameters)
    torch.manual_seed(8)
    y, h = fused(x, res, (shape[-1], ), *parameters, eps=EPS, p=p, bits=bits, prenorm=True)
    grads = torch.autograd.grad(y, leaves, gy)
    assert len(seeds) == 2 and type(y.grad_fn).__name__ == plain.node                 # the dropout's seed, then the norm's
    torch.manual_seed(8)
    h0 = fewbit.functional.dropout_add(x, res, p, True)
    y0 = plain.functional(h0, (shape[-1], ), *parameters, EPS, bits)
    assert torch.equal(y, y0) and torch.equal(h, h0) and all(torch.equal(a, b) for a, b in zip(grads, torch.autograd.grad(y0, leaves, gy)))


@pytest.mark.parametrize('name', KINDS)
def test_grad_mode_off_still_drops_and_eval_gives_torchs_exact_gradients(name, seeds):
    plain, fused, module = KINDS[name]
    shape, dtype, p = SHAPES[0], torch.bfloat16, 0.5
    x, parameters, gy = harness.problem(plain, shape, dtype, 4)
    res = residual_of(shape, dtype)
    layer = module(shape[-1], eps=EPS, device=DEV, dtype=dtype, p=p, prenorm=True)
    with torch.no_grad():
        for t, value in zip(layer.parameters(), parameters):
            t.copy_(value)
        (y, h), saved = saved_by(lambda: layer(x, res))
    assert y.grad_fn is None and not saved and len(seeds) == 1            # the plain fused forward: one seed for the mask, no state
    flat = lambda t: t.detach().reshape(-1, shape[-1])
    he = cabi_x.dropout_apply(flat(x).contiguous(), seeds[0], p, addend=flat(res).contiguous())
    assert torch.equal(h, he.view(shape)) and torch.equal(y, plain.forward(he, *(t.detach() for t in layer.parameters()), EPS, keep=False)[0].view(shape))
    layer.eval()
    (y, h), saved = saved_by(lambda: layer(x, res))
    assert len(seeds) == 1 and 'Quantized' not in type(y.grad_fn).__name__ and not any(t.dtype == torch.uint8 for t in saved)
    norm = F.layer_norm if plain.centred else F.rms_norm
    want = norm(res + x, (shape[-1], ), *layer.parameters(), EPS)
    assert torch.equal(h, res + x) and torch.equal(y, want)
    assert all(torch.equal(a, b) for a, b in zip(torch.autograd.grad(y, (x, res), gy), torch.autograd.grad(want, (x, res), gy)))
    with torch.no_grad():
        y2, h2 = layer(x, res)                                            # eval without grad: the fused forward without a mask, no seed
    assert len(seeds) == 1 and torch.equal(h2, res + x) and torch.equal(y2, plain.forward(flat(res + x), *(t.detach() for t in layer.parameters()), EPS, keep=False)[0].view(shape))


# ---- inside training wrappers: the shared bodies of the harness on the layer with its residual bound ----------------------------------------------
@pytest.mark.parametrize('reentrant', (False, True), ids=('non_reentrant', 'reentrant'))
@pytest.mark.parametrize('name', KINDS)
def test_checkpointing_gives_the_plain_runs_bits(name, reentrant):
    harness.checkpointing_gives_the_plain_runs_bits(bound(name, SHAPES[0], 0.1), SHAPES[0], reentrant)


@pytest.mark.parametrize('name', KINDS)
def test_backward_may_follow_the_autocast_block(name, seeds):
    harness.backward_may_follow_the_autocast_block(bound(name, SHAPES[0], 0.1), SHAPES[0], seeds)


@pytest.mark.parametrize('name', KINDS)
def test_no_grad_eval_and_frozen_parameters_build_no_node_and_keep_no_state(name, seeds):
    """(without a mask: the body compares the outputs of several calls, which a mask of a fresh seed per call would tell apart)"""
    kind = bound(name, SHAPES[0], 0.0)
    x, _, _ = harness.problem(kind, SHAPES[0], torch.bfloat16, 3)
    harness.no_grad_eval_and_frozen_parameters_build_no_node_and_keep_no_state(kind, x, seeds)


@pytest.mark.parametrize('name', KINDS)
def test_a_captured_step_draws_fresh_masks_and_roundings_on_every_replay(name, monkeypatch):
    harness.a_captured_step_rounds_afresh_on_every_replay(bound(name, SHAPES[0], 0.1), SHAPES[0], monkeypatch)
