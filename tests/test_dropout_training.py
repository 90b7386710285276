"""``fewbit.Dropout`` / ``dropout`` / ``dropout_add`` the way a training script runs them: inside both modes of ``torch.utils.checkpoint``, under
autocast with ``backward()`` inside and after the block, one module called twice, ``no_grad`` / ``inference_mode`` evaluation, in place on views
and leaves, and at the edges of the argument list.

This file runs the autograd node ``_SeededDropout`` on HOST tensors: the fixture ``host_node`` lets ``dropout._kernel_applies`` accept them and
puts the definition, evaluated by torch, where the kernel binding is (``cabi_x.dropout_apply``: the mask from ``cabi_x.dropout_keep``, the
arithmetic of ``reference()`` in tests/test_gpu_dropout.py).  Everything else is the shipped code.  tests/test_gpu_dropout_training.py runs
the ``check_*`` functions below on the gfx950 kernel.  Every value is compared bit for bit with that definition for the seed the call drew
(recorded through ``linear._draw_seed``); two runs that are compared start from the same ``torch.manual_seed``.  Nothing is statistical."""
import contextlib
import copy
import importlib
import pickle

import numpy
import pytest
import torch
from torch.utils.checkpoint import checkpoint

import fewbit
from fewbit_amd import cabi_x, linear
from fewbit_amd.linear import LinearGRP
from fewbit_amd.variance import VarianceEstimator
from test_gpu_dropout import ONE, assert_same, reference

drop = importlib.import_module('fewbit_amd.dropout')                 # (the package attribute of that name is the function)
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
RUN_SEED = 7
ROWS, WIDTH = 8, 16
SHAPE = (ROWS, WIDTH)                                                # (the GPU file passes its own)


def expected(x, r, seed, p):
    """the definition for ``seed`` on host copies of ``x`` and ``r`` (or None) -> host tensor of x's dtype"""
    threshold = cabi_x.dropout_threshold(p)
    x = x.detach().cpu().contiguous()
    keep = cabi_x.dropout_keep(seed, x.numel(), p).view(x.shape)
    return reference(x, None if r is None else r.detach().cpu().contiguous(), keep, threshold)


def keep_of(seed, shape, p):
    n = 1
    for s in shape:
        n *= s
    return cabi_x.dropout_keep(seed, n, p).view(shape)


def scale_of(p):
    return float(torch.tensor(65536.0 / (ONE - cabi_x.dropout_threshold(p)), dtype=torch.float64).float())


def host_apply(src, seed, p, addend=None, out=None, first=0, stream=None):
    """``cabi_x.dropout_apply`` on host tensors: the same refusals, the definition evaluated by torch"""
    assert src.device.type == 'cpu' and src.dtype in DTYPES and src.is_contiguous() and isinstance(seed, int) and first == 0
    assert addend is None or (addend.shape == src.shape and addend.dtype == src.dtype and addend.is_contiguous())
    threshold = cabi_x.dropout_threshold(p)
    if threshold == ONE:                                             # (the scale is infinite: every element is dropped)
        want = torch.zeros_like(src) if addend is None else addend.clone()
    else:
        want = reference(src.detach(), None if addend is None else addend.detach(), cabi_x.dropout_keep(seed, src.numel(), p).view(src.shape), threshold)
    if out is None:
        return want
    assert out.shape == src.shape and out.dtype == src.dtype and out.is_contiguous()
    out.copy_(want)
    return out


def record_seeds(monkeypatch):
    """-> the list of the seeds drawn through ``linear._draw_seed`` from here on, in order"""
    drawn, real = [], linear._draw_seed

    def draw(generator):
        drawn.append(real(generator))
        return drawn[-1]

    monkeypatch.setattr(linear, '_draw_seed', draw)
    return drawn


@pytest.fixture
def seeds(monkeypatch):
    return record_seeds(monkeypatch)


@pytest.fixture
def host_node(monkeypatch, seeds):
    """``_SeededDropout`` on host tensors (module docstring) -> the recorded seeds"""
    monkeypatch.setattr(drop, '_kernel_applies', lambda t: t.device.type == 'cpu' and t.dtype in DTYPES and t.numel() > 0)
    monkeypatch.setattr(cabi_x, 'dropout_apply', host_apply)
    monkeypatch.setattr(linear, '_sketch_seed', lambda generator, device: linear._draw_seed(generator))
    return seeds


# ---- the block ----------------------------------------------------------------------------------------------------------------------------
def make_block(device, inplace=False, p=0.5, width=WIDTH):
    g = torch.Generator().manual_seed(11)
    block = torch.nn.Sequential(torch.nn.Linear(width, width), fewbit.Dropout(p, inplace), torch.nn.Linear(width, width))
    with torch.no_grad():
        for t in block.parameters():
            t.copy_(torch.randn(t.shape, generator=g) * 0.3)
    return block.to(device)


def block_data(device, shape=SHAPE, seed=1):
    """-> (x, w): the input and the fixed fp32 weights of the loss ``(y.float() * w).sum()``"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(device), torch.randn(*shape, generator=g).to(device)


def run_block(block, x, w, forward=None, amp=None, backward_inside=True):
    """one step from ``torch.manual_seed(RUN_SEED)`` -> (y, [x.grad, the four parameter gradients], the host RNG state after backward)"""
    block.zero_grad()
    xi = x.detach().clone().requires_grad_()
    torch.manual_seed(RUN_SEED)
    ctx = torch.autocast(xi.device.type, dtype=amp) if amp is not None else contextlib.nullcontext()
    with ctx:
        y = block(xi) if forward is None else forward(block, xi)
        loss = (y.float() * w).sum()
        if backward_inside:
            loss.backward()
    if not backward_inside:
        loss.backward()
    return y.detach(), [xi.grad] + [t.grad for t in block.parameters()], torch.get_rng_state()


def assert_equal_runs(got, want, what):
    assert torch.equal(got[0], want[0]) and got[0].dtype == want[0].dtype, (what, 'output')
    assert len(got[1]) == len(want[1]) == 5
    for k, (a, b) in enumerate(zip(got[1], want[1])):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (what, 'gradient', k, float((a.float() - b.float()).abs().max()))


def check_plain_block_is_the_definition(device, seeds, inplace=False, amp=None, shape=SHAPE):
    """the plain run against an autograd graph of torch operators built on the host mask of the recorded seed: the output and all five gradients"""
    block, (x, w) = make_block(device, inplace, width=shape[-1]), block_data(device, shape)
    del seeds[:]
    plain = run_block(block, x, w, amp=amp)
    assert len(seeds) == 1
    keep, scale = keep_of(seeds[0], shape, 0.5).to(device), scale_of(0.5)

    def by_torch(m, xi):
        h = m[0](xi)
        d = torch.where(keep, h.float() * scale, torch.zeros((), device=device)).to(h.dtype)
        return m[2](d)

    assert_equal_runs(run_block(block, x, w, forward=by_torch, amp=amp), plain, 'the block against torch operators on the host mask')
    assert int(torch.count_nonzero(plain[1][1])) > 0 and len(seeds) == 1
    return plain


# ---- 1. checkpointing -------------------------------------------------------------------------------------------------------------------
def check_checkpointed_block(device, seeds, reentrant, inplace, amp=None, backward_inside=True, generator=None, shape=SHAPE):
    """``checkpoint(block, x)`` after the same ``torch.manual_seed``: the output, the input gradient and the four parameter gradients are the
    plain run's; the seed seam is called twice -- forward and recomputation -- with one value; the host RNG ends where the plain run's does"""
    block, (x, w) = make_block(device, inplace, width=shape[-1]), block_data(device, shape)
    block[1].generator = generator
    del seeds[:]
    plain = run_block(block, x, w, amp=amp)
    assert len(seeds) == 1
    del seeds[:]
    ckpt = run_block(block, x, w, forward=lambda m, xi: checkpoint(m, xi, use_reentrant=reentrant), amp=amp, backward_inside=backward_inside)
    assert len(seeds) == 2 and seeds[0] == seeds[1], seeds
    assert_equal_runs(ckpt, plain, f'checkpoint(use_reentrant={reentrant}), inplace={inplace}')
    assert torch.equal(ckpt[2], plain[2]), 'the host generator ends elsewhere than after the plain run'
    return plain, ckpt


@pytest.mark.parametrize('inplace', (False, True), ids=('out-of-place', 'inplace'))
@pytest.mark.parametrize('reentrant', (False, True), ids=('non-reentrant', 'reentrant'))
def test_a_checkpointed_block_gives_the_plain_runs_bits(reentrant, inplace, host_node):
    check_plain_block_is_the_definition('cpu', host_node, inplace)
    check_checkpointed_block('cpu', host_node, reentrant, inplace)


# ---- 2. autocast --------------------------------------------------------------------------------------------------------------------------
def check_autocast(device, seeds, amp, shape=SHAPE):
    """under autocast: ``dropout(h)`` of a 16-bit ``h`` stays 16-bit, ``dropout_add(h, r_fp32)`` takes the composed form and is fp32,
    ``dropout_add(h, h)`` is 16-bit; each is the definition for its own seed; ``backward()`` after the block gives the bits of ``backward()``
    inside it and the leaf gradients are fp32"""
    block, (x, w) = make_block(device, width=shape[-1]), block_data(device, shape)
    seen = {}

    def forward(m, xi):
        h = m[0](xi)
        a = fewbit.functional.dropout(h, 0.5)
        b = fewbit.functional.dropout_add(a, a, 0.25)
        c = fewbit.functional.dropout_add(b, xi, 0.5)
        seen.update(h=h.detach(), a=a.detach(), b=b.detach(), c=c.detach())
        return m[2](c)

    del seeds[:]
    inside = run_block(block, x, w, forward=forward, amp=amp, backward_inside=True)
    assert len(seeds) == 3 and len(set(seeds)) == 3
    assert seen['h'].dtype == amp and seen['a'].dtype == amp and seen['b'].dtype == amp and seen['c'].dtype == torch.float32 and inside[0].dtype == amp
    assert_same(seen['a'], expected(seen['h'], None, seeds[0], 0.5), 'dropout(h) under autocast')
    assert_same(seen['b'], expected(seen['a'], seen['a'], seeds[1], 0.25), 'dropout_add(h, h) under autocast')
    assert_same(seen['c'], x.cpu() + expected(seen['b'], None, seeds[2], 0.5), 'dropout_add(h, r_fp32) under autocast: the composed form')
    first = list(seeds)
    del seeds[:]
    outside = run_block(block, x, w, forward=forward, amp=amp, backward_inside=False)
    assert seeds == first
    assert_equal_runs(outside, inside, 'backward() after the autocast block against inside it')
    assert all(g.dtype == torch.float32 for g in outside[1]) and int(torch.count_nonzero(outside[1][0])) > 0


def test_autocast_dtypes_and_backward_after_the_block(host_node):
    check_autocast('cpu', host_node, torch.bfloat16)
    check_plain_block_is_the_definition('cpu', host_node, amp=torch.bfloat16)


# ---- 3. one tensor twice, retained graphs, second order, gradients that are not contiguous -----------------------------------------------
def check_same_tensor_twice(device, seeds, dtype=torch.float32, shape=SHAPE):
    """``dropout_add(h, h, p)`` with ``h = x * 1``: both gradients of the node reach x, ``where(keep, 1 + scale, 1)``"""
    x = block_data(device, shape)[0].to(dtype).requires_grad_()
    h = x * 1
    del seeds[:]
    y = fewbit.functional.dropout_add(h, h, 0.25)
    assert len(seeds) == 1 and y.dtype == dtype
    assert_same(y.detach(), expected(h, h, seeds[0], 0.25), 'dropout_add(h, h)')
    y.sum().backward()
    ones = torch.ones(x.shape, dtype=dtype)
    want = ones + expected(ones, None, seeds[0], 0.25)               # (the two gradients are added in the dtype, as autograd adds them)
    assert_same(x.grad, want, 'the gradient of dropout_add(h, h)')
    keep = keep_of(seeds[0], x.shape, 0.25)
    if dtype == torch.float32:
        assert torch.equal(x.grad.cpu(), torch.where(keep, torch.tensor(1 + scale_of(0.25)), torch.tensor(1.0)))


def test_dropout_add_of_one_tensor_with_itself(host_node):
    check_same_tensor_twice('cpu', host_node)


def check_retained_graph(device, seeds, shape=SHAPE):
    block, (x, w) = make_block(device, width=shape[-1]), block_data(device, shape)
    xi = x.clone().requires_grad_()
    del seeds[:]
    loss = (block(xi) * w).sum()
    loss.backward(retain_graph=True)
    first = [xi.grad.clone()] + [t.grad.clone() for t in block.parameters()]
    block.zero_grad()
    xi.grad = None
    loss.backward()
    assert len(seeds) == 1 and int(torch.count_nonzero(first[0])) > 0
    for a, b in zip([xi.grad] + [t.grad for t in block.parameters()], first):
        assert torch.equal(a, b)


def test_a_second_backward_through_a_retained_graph_gives_the_same_bits(host_node):
    check_retained_graph('cpu', host_node)


def test_a_second_order_backward_raises(host_node):
    x = block_data('cpu')[0].requires_grad_()
    y = fewbit.functional.dropout(x, 0.5)
    (gx, ) = torch.autograd.grad(y.square().sum(), x, create_graph=True)          # (a gradient penalty: grad_output = 2 y is part of the graph)
    with pytest.raises(RuntimeError, match='once_differentiable'):
        gx.sum().backward()


def check_strided_grad_output(device, seeds, shape=SHAPE):
    """the expanded (0-stride) gradient of ``y.sum()`` and a transposed one give the bits of their contiguous copies -- the definition's"""
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(3)).to(device).requires_grad_()

    def run(backward):
        x.grad = None
        torch.manual_seed(RUN_SEED)
        del seeds[:]
        backward(fewbit.functional.dropout(x, 0.5))
        return x.grad

    ones = torch.ones(shape)
    assert_same(run(lambda y: y.sum().backward()), expected(ones, None, seeds[0], 0.5), 'the expanded gradient of y.sum()')
    gy = torch.randn(shape[-1], *shape[:-1], generator=torch.Generator().manual_seed(4)).to(device).movedim(0, -1)
    assert gy.shape == tuple(shape) and not gy.is_contiguous()
    got = run(lambda y: y.backward(gy))
    assert_same(got, expected(gy.contiguous(), None, seeds[0], 0.5), 'a transposed grad_output')
    assert torch.equal(got, run(lambda y: y.backward(gy.contiguous())))


def test_a_grad_output_that_is_not_contiguous(host_node):
    check_strided_grad_output('cpu', host_node)


def check_one_module_called_twice(device, seeds, dtype=torch.float32, shape=SHAPE):
    """one module on two tensors in one step: two seeds, two masks, each backward meets its own"""
    m = fewbit.Dropout(0.5)
    g = torch.Generator().manual_seed(5)
    x1, x2 = (torch.randn(*shape, generator=g).to(dtype).to(device).requires_grad_() for _ in range(2))
    g1, g2 = (torch.randn(*shape, generator=g).to(dtype).to(device) for _ in range(2))
    del seeds[:]
    y1, y2 = m(x1), m(x2)
    assert len(seeds) == 2 and seeds[0] != seeds[1]
    assert not torch.equal(keep_of(seeds[0], shape, 0.5), keep_of(seeds[1], shape, 0.5))
    assert_same(y1.detach(), expected(x1, None, seeds[0], 0.5), 'the first call')
    assert_same(y2.detach(), expected(x2, None, seeds[1], 0.5), 'the second call')
    ((y1 * g1).sum() + (y2 * g2).sum()).backward()
    assert_same(x1.grad, expected(g1, None, seeds[0], 0.5), 'the gradient of the first call')
    assert_same(x2.grad, expected(g2, None, seeds[1], 0.5), 'the gradient of the second call')
    assert len(seeds) == 2


def test_one_module_called_twice_draws_two_seeds_and_two_masks(host_node):
    check_one_module_called_twice('cpu', host_node)


# ---- 4. no gradient -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ('no_grad', 'inference_mode', 'nothing requires grad'))
def test_without_a_gradient_it_still_drops_builds_no_node_and_draws_one_seed(mode, host_node):
    x = block_data('cpu')[0].requires_grad_(mode != 'nothing requires grad')
    m = fewbit.Dropout(0.5)
    with {'no_grad': torch.no_grad, 'inference_mode': torch.inference_mode}.get(mode, contextlib.nullcontext)():
        y = m(x)
    assert len(host_node) == 1 and y.grad_fn is None and not y.requires_grad and y is not x
    assert_same(y, expected(x, None, host_node[0], 0.5), mode)
    assert int((y == 0).sum()) > 0


def test_eval_and_p_zero_return_the_input_and_draw_nothing(host_node):
    x = block_data('cpu')[0].requires_grad_()
    r = torch.ones_like(x)
    before = torch.get_rng_state()
    assert fewbit.Dropout(0.5).eval()(x) is x and fewbit.Dropout(0.0)(x) is x and fewbit.functional.dropout(x, 0.5, training=False) is x
    assert fewbit.functional.dropout(x, 2.0**-18) is x               # (a threshold of 0)
    assert torch.equal(fewbit.functional.dropout_add(x, r, 0.0), r + x) and torch.equal(fewbit.functional.dropout_add(x, r, 0.5, training=False), r + x)
    assert host_node == [] and torch.equal(torch.get_rng_state(), before)


# ---- 5. in place --------------------------------------------------------------------------------------------------------------------------
def check_in_place_on_a_view(device, seeds):
    """in place on the left half of a non-leaf: the model's values there, the right half untouched, the gradient through the base is right"""
    x = block_data(device)[0].requires_grad_()
    h = x * 1
    was = h.detach().clone()
    view = h[:, :WIDTH // 2]
    del seeds[:]
    out = fewbit.functional.dropout(view, 0.5, inplace=True)
    assert len(seeds) == 1 and out.data_ptr() == h.data_ptr() and out.shape == view.shape
    assert_same(h.detach()[:, :WIDTH // 2].contiguous(), expected(was[:, :WIDTH // 2], None, seeds[0], 0.5), 'the written half')
    assert torch.equal(h.detach()[:, WIDTH // 2:], was[:, WIDTH // 2:])
    g = torch.randn(ROWS, WIDTH, generator=torch.Generator().manual_seed(6)).to(device)
    (h * g).sum().backward()
    want = torch.cat((expected(g[:, :WIDTH // 2], None, seeds[0], 0.5), g[:, WIDTH // 2:].cpu()), dim=1)
    assert_same(x.grad, want, 'the gradient through the base')


def test_in_place_on_a_view_of_a_non_leaf(host_node):
    check_in_place_on_a_view('cpu', host_node)


def check_in_place_without_grad_returns_the_input(device, seeds, dtype=torch.float32, shape=SHAPE):
    """``dropout(x, inplace=True)`` under ``no_grad`` on a leaf that requires grad: the input object itself, still requiring grad, holding the
    definition's values, as ``torch.nn.functional.dropout`` does (``x = drop(x)`` must not stop x from requiring grad)"""
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(8)).to(dtype).to(device).requires_grad_()
    was, version = x.detach().clone(), x._version
    ref = x.detach().clone().requires_grad_()
    with torch.no_grad():
        assert torch.nn.functional.dropout(ref, 0.5, inplace=True) is ref and ref.requires_grad       # (what torch does)
        del seeds[:]
        y = fewbit.Dropout(0.5, inplace=True)(x)
    assert y is x, 'another tensor object came back'
    assert x.requires_grad and x.is_leaf and x.grad_fn is None and x._version > version
    assert len(seeds) == 1
    assert_same(x.detach(), expected(was, None, seeds[0], 0.5), 'in place under no_grad')
    # a transposed leaf: written through its strides
    t = torch.randn(shape[-1], shape[0], generator=torch.Generator().manual_seed(9)).to(dtype).to(device).t().requires_grad_()
    was = t.detach().clone()
    with torch.no_grad():
        assert fewbit.functional.dropout(t, 0.5, inplace=True) is t and t.requires_grad
    assert_same(t.detach().contiguous(), expected(was.contiguous(), None, seeds[1], 0.5), 'in place under no_grad, transposed')
    # with grad mode on it is refused before anything is written, as in torch
    with pytest.raises(RuntimeError, match='leaf Variable'):
        fewbit.functional.dropout(x, 0.5, inplace=True)
    assert len(seeds) == 2


def test_in_place_under_no_grad_returns_the_input_object_itself(host_node):
    check_in_place_without_grad_returns_the_input('cpu', host_node)
    x = torch.ones(ROWS, WIDTH)
    with torch.inference_mode():
        assert fewbit.functional.dropout(x, 0.5, inplace=True) is x
    assert_same(x, expected(torch.ones(ROWS, WIDTH), None, host_node[-1], 0.5), 'in place under inference_mode')


# ---- 6. arguments and copies ----------------------------------------------------------------------------------------------------------
def test_p_as_a_numpy_scalar_p_as_the_int_one_and_a_0d_input(host_node):
    x = block_data('cpu')[0].requires_grad_()
    y = fewbit.functional.dropout(x, numpy.float32(0.5))
    assert_same(y.detach(), expected(x, None, host_node[0], 0.5), 'p = numpy.float32(0.5)')
    y.sum().backward()
    assert_same(x.grad, expected(torch.ones_like(x), None, host_node[0], 0.5), 'its gradient')
    x.grad = None
    z = fewbit.Dropout(1)(x)
    z.sum().backward()
    assert z.dtype == x.dtype and not bool(z.detach().view(torch.int32).any()) and not bool(x.grad.view(torch.int32).any())
    r = torch.ones_like(x)
    assert torch.equal(fewbit.functional.dropout_add(x, r, 1), r)
    s = torch.tensor(3.0, requires_grad=True)
    del host_node[:]
    outs = [fewbit.functional.dropout(s, 0.5) for _ in range(8)]
    assert all(o.shape == () for o in outs) and len(host_node) == 8
    for o, seed in zip(outs, host_node):
        assert_same(o.detach(), expected(s, None, seed, 0.5), 'a 0-d input')
    sum(outs).backward()
    assert float(s.grad) == 2.0 * sum(bool(cabi_x.dropout_keep(seed, 1, 0.5)[0]) for seed in host_node)


def test_deepcopy_and_pickle_of_a_module_with_a_generator(host_node):
    m = fewbit.Dropout(0.1, generator=torch.Generator().manual_seed(21))
    x = block_data('cpu')[0]
    for other in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert type(other) is fewbit.Dropout and other.p == 0.1 and other.inplace is False and other.generator is not m.generator
        assert torch.equal(other.generator.get_state(), m.generator.get_state())
        del host_node[:]
        y = other(x)                                                 # (the copy draws from its own generator: the original's does not move)
        assert len(host_node) == 1 and torch.equal(other.generator.get_state(), m.generator.get_state()) is False
        assert_same(y, expected(x, None, host_node[0], 0.1), 'the copy')
    first = host_node[0]
    del host_node[:]
    m(x)
    assert host_node == [first]                                      # the same stream from the same state


def test_torch_func_grad_and_vmap_are_refused_with_torchs_own_message(host_node):
    """the node has no ``setup_context`` (it keeps its seed in ``ctx`` inside forward): function transforms say so by name"""
    x = block_data('cpu')[0]
    with pytest.raises(RuntimeError, match='setup_context'):
        torch.func.grad(lambda t: fewbit.functional.dropout(t, 0.5).sum())(x)
    with pytest.raises(RuntimeError, match='setup_context'):
        torch.vmap(lambda t: fewbit.functional.dropout(t, 0.5))(x)


# ---- 7. a whole sublayer of this package ------------------------------------------------------------------------------------------------
SUB_SHAPE, SUB_P = (2, 19, 24), 0.1


class Sublayer(torch.nn.Module):
    """a transformer sublayer built from this package: an estimator-wrapped randomized linear, the few-bit GELU, a linear, the seeded dropout
    and ``dropout_add`` with the sublayer's input"""

    def __init__(self):
        super().__init__()
        self.fc1 = VarianceEstimator(LinearGRP(24, 48, proj_dim=5, matmul='rademacher'))
        self.act = fewbit.GELU(bits=3)
        self.fc2 = torch.nn.Linear(48, 24)
        self.drop = fewbit.Dropout(SUB_P)
        g = torch.Generator().manual_seed(13)
        with torch.no_grad():
            for t in self.parameters():
                t.copy_(torch.randn(t.shape, generator=g) * 0.3)

    def forward(self, x):
        h = self.drop(self.fc2(self.act(self.fc1(x))))
        return fewbit.functional.dropout_add(h, x, SUB_P)


def check_sublayer(device, seeds, amp, draws=2, saved_bytes=False):
    """the sublayer plain, and inside a non-reentrant checkpoint with ``backward()`` after the autocast block, from the same ``torch.manual_seed``:
    the same loss and gradients bit for bit, the same seeds in the same order (layer, dropout, dropout_add), one estimator triple per step equal
    to the plain run's; the module's dropout is the definition for ITS seed; swapping it for ``nn.Dropout`` and back moves the saved bytes by
    one byte per element.  ``draws``: the seeds of one forward -- 2 on the host, where the layer's PyTorch formulation draws through
    ``_capture_rng``, 3 on the kernels; ``saved_bytes``: on the GPU, where torch's dropout saves one bool per element (its host formulation saves an fp32 mask)"""
    m = Sublayer().to(device)
    x, w = block_data(device, SUB_SHAPE)
    seen = []
    hook = m.drop.register_forward_hook(lambda mod, args, out: seen.append((args[0].detach().clone(), out.detach().clone())))

    def run(forward, backward_inside):
        m.zero_grad()
        xi = x.clone().requires_grad_()
        torch.manual_seed(RUN_SEED)
        del seeds[:]
        before = m.fc1.state.step
        with torch.autocast(torch.device(device).type, dtype=amp) if amp is not None else contextlib.nullcontext():
            y = forward(xi)
            loss = (y.float() * w).sum()
            if backward_inside:
                loss.backward()
        if not backward_inside:
            loss.backward()
        return loss.detach(), [xi.grad] + [t.grad for t in m.parameters()], list(seeds), m.fc1.variance, m.fc1.state.step - before

    plain = run(m, True)
    assert len(plain[2]) == draws and len(set(plain[2])) == draws and plain[4] == 1
    h_in, h_out = seen[0]
    assert h_in.dtype == (amp or torch.float32) and h_in.shape == SUB_SHAPE
    assert_same(h_out, expected(h_in, None, plain[2][-2], SUB_P), 'the dropout module inside the sublayer')
    ckpt = run(lambda xi: checkpoint(m, xi, use_reentrant=False), False)
    hook.remove()
    assert torch.equal(ckpt[0], plain[0]), (float(ckpt[0]), float(plain[0]))
    for k, (a, b) in enumerate(zip(ckpt[1], plain[1])):
        assert a.dtype == b.dtype == torch.float32 and torch.equal(a, b) and int(torch.count_nonzero(a)) > 0, ('gradient', k)
    # forward draws the plain run's seeds; the recomputation draws them again from the start (it may stop early: the dropout nodes save nothing)
    assert ckpt[2][:draws] == plain[2] and len(ckpt[2]) <= 2 * draws and ckpt[2][draws:] == plain[2][:len(ckpt[2]) - draws], (ckpt[2], plain[2])
    assert ckpt[4] == 1 and all(torch.equal(a, b) and bool(torch.isfinite(a)) for a, b in zip(ckpt[3], plain[3])), (ckpt[3], plain[3])
    assert m.fc1.state.bs == 38 and m.fc1.state.bs_proj == 5 and torch.equal(m.fc1.state.input, x)
    if not saved_bytes:
        return

    def saved():
        with fewbit.memory_usage_hooks() as usage:
            m(x.clone().requires_grad_())
        return usage.forward

    ours = saved()
    fewbit.map_module(m, lambda mod, path: torch.nn.Dropout(mod.p, mod.inplace) if type(mod) is fewbit.Dropout else mod)
    assert type(m.drop) is torch.nn.Dropout
    theirs = saved()
    fewbit.map_module(m, lambda mod, path: fewbit.Dropout(mod.p, mod.inplace) if type(mod) is torch.nn.Dropout else mod)
    assert type(m.drop) is fewbit.Dropout
    assert theirs - ours == 2 * 19 * 24 and saved() == ours, (ours, theirs)


@pytest.mark.parametrize('amp', (None, torch.bfloat16), ids=('plain', 'bf16-autocast'))
def test_a_sublayer_of_this_package_checkpointed_with_backward_after_the_autocast_block(amp, host_node):
    check_sublayer('cpu', host_node, amp)
