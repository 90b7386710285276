"""LinearGRP / LinearCRS the way a training script runs them: under autocast with ``backward()`` inside AND after the block, under both modes
of ``torch.utils.checkpoint``, under ``no_grad`` / ``inference_mode`` / a frozen weight, and at the edges of a batch (no rows, one row, a
gradient that is not unit-stride, two backward passes, one layer called twice, an overflowed gradient).

This file runs the PyTorch formulation on the host; tests/test_gpu_linear_training.py runs the same checks (the ``check_*`` functions below)
on the gfx950 kernels.  Nothing here is statistical: where two runs are compared the seed is pinned (``torch.manual_seed`` before each run:
the layer's seed is one draw from the host default generator) and "equal" is ``torch.equal`` -- the same seed gives the same S, rows or
columns, and the library GEMMs are called with identical arguments."""
import collections
import contextlib

import pytest
import torch
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint

from fewbit_amd import linear
from fewbit_amd.linear import LinearCRS, LinearGRP


class Route:
    """one way through the layer: the estimator, the input's shape (rows..., without the features), the widths, proj_dim, the row switch"""

    def __init__(self, name, kind, shape, fin, fout, proj, extend=False):
        self.name, self.kind, self.shape, self.fin, self.fout, self.proj, self.extend = name, kind, tuple(shape), fin, fout, proj, extend

    def __repr__(self):
        return self.name

    def enter(self):
        """set the row-extension switch this route needs (the caller's fixture restores it)"""
        linear.use_row_extension(self.extend)

    def layer(self, device, dtype=torch.float32, generator=None):
        if self.kind == 'crs':
            m = LinearCRS(self.fin, self.fout, proj_dim=self.proj, device=device, dtype=dtype)
        else:
            m = LinearGRP(self.fin, self.fout, proj_dim=self.proj, matmul=self.kind, generator=generator, device=device, dtype=dtype)
        g = torch.Generator().manual_seed(11)
        with torch.no_grad():
            m.weight.copy_((torch.randn(self.fout, self.fin, generator=g) * 0.2).to(dtype))
            m.bias.copy_(torch.randn(self.fout, generator=g).to(dtype))
        return m

    def data(self, device, dtype=torch.float32, shape=None, seed=1):
        """-> (x, w): the input and the fixed fp32 weights of the loss ``(y.float() * w).sum()`` (so ``grad_output`` is ``w`` in y's dtype)"""
        shape = self.shape if shape is None else tuple(shape)
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(*shape, self.fin, generator=g).to(dtype).to(device)
        w = torch.randn(*shape, self.fout, generator=g).to(device)
        return x, w


HOST_ROUTES = [Route(kind, kind, (96, ), 48, 24, 24) for kind in ('gaussian', 'rademacher', 'dct', 'dft')] + [Route('crs', 'crs', (96, ), 48, 24, 24)]
RUN_SEED = 7


@pytest.fixture(autouse=True)
def switches_restored():
    native, extend = linear.use_native_sketch(), linear.use_row_extension()
    yield
    linear.use_native_sketch(native)
    linear.use_row_extension(extend)


def grads(layer, x):
    return [t.grad for t in (layer.weight, layer.bias, x)]


def step(layer, x, w, forward=None, amp=None, backward_inside=True, seed=RUN_SEED):
    """one training step from ``torch.manual_seed(seed)``: -> (y, [weight.grad, bias.grad, input.grad]); ``forward``: how the layer is called
    (default: ``layer(x)``); ``amp``: the autocast dtype, with ``backward()`` inside the block or after it"""
    layer.zero_grad()
    xi = x.detach().clone().requires_grad_()
    torch.manual_seed(seed)
    block = torch.autocast(xi.device.type, dtype=amp) if amp is not None else contextlib.nullcontext()
    with block:
        y = layer(xi) if forward is None else forward(layer, xi)
        loss = (y.float() * w).sum()
        if backward_inside:
            loss.backward()
    if not backward_inside:
        loss.backward()
    return y.detach(), grads(layer, xi)


def assert_same_bits(got, want, what):
    for name, a, b in zip(('weight.grad', 'bias.grad', 'input.grad'), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype)
        assert torch.equal(a, b), (what, name, float((a.float() - b.float()).abs().max()))


# ---- 1. backward() after the autocast block ---------------------------------------------------------------------------------------------
def check_backward_outside_autocast(route, device, in_dtype, amp=torch.bfloat16):
    """an fp32 layer under autocast, fp32 input (a first layer) or 16-bit input (an inner layer): ``backward()`` after the block does not
    raise and gives the bits of ``backward()`` inside it; the gradients have the dtypes of their leaves"""
    route.enter()
    layer = route.layer(device)
    x, w = route.data(device, in_dtype)
    y_in, inside = step(layer, x, w, amp=amp, backward_inside=True)
    y_out, outside = step(layer, x, w, amp=amp, backward_inside=False)
    assert y_in.dtype == amp and y_out.dtype == amp and torch.equal(y_in, y_out)
    assert [t.dtype for t in outside] == [torch.float32, torch.float32, in_dtype]
    assert outside[0].shape == layer.weight.shape and int(torch.count_nonzero(outside[0])) > 0
    assert_same_bits(outside, inside, f'{route}: backward() after the autocast block against inside it')


@pytest.mark.parametrize('in_dtype', (torch.float32, torch.bfloat16), ids=('fp32-input', 'bf16-input'))
@pytest.mark.parametrize('route', HOST_ROUTES, ids=repr)
def test_backward_after_the_autocast_block_equals_backward_inside_it(route, in_dtype):
    check_backward_outside_autocast(route, 'cpu', in_dtype)


def test_a_backward_without_autocast_in_forward_ignores_the_callers_autocast():
    """forward outside any autocast block, ``backward()`` called inside one: the gradient is the plain run's (the forward's state is what
    counts, as with torch.amp.custom_bwd)"""
    for route in HOST_ROUTES:
        layer = route.layer('cpu')
        x, w = route.data('cpu')
        _, plain = step(layer, x, w)
        layer.zero_grad()
        xi = x.clone().requires_grad_()
        torch.manual_seed(RUN_SEED)
        loss = (layer(xi) * w).sum()
        with torch.autocast('cpu', dtype=torch.bfloat16):
            loss.backward()
        assert_same_bits(grads(layer, xi), plain, f'{route}: backward() inside a block the forward did not see')


# ---- 3. checkpointing -----------------------------------------------------------------------------------------------------------------
def check_checkpointing(route, device, reentrant, amp=None, in_dtype=torch.float32):
    """``checkpoint(layer, x)`` after the same ``torch.manual_seed`` as a plain run: it runs, and all three gradients are the plain run's"""
    route.enter()
    layer = route.layer(device)
    x, w = route.data(device, in_dtype)
    y, plain = step(layer, x, w, amp=amp)
    yc, ckpt = step(layer, x, w, forward=lambda m, xi: checkpoint(m, xi, use_reentrant=reentrant), amp=amp)
    assert torch.equal(y, yc) and int(torch.count_nonzero(plain[0])) > 0
    assert_same_bits(ckpt, plain, f'{route}: checkpoint(use_reentrant={reentrant}) against the plain run')


@pytest.mark.parametrize('reentrant', (False, True), ids=('non-reentrant', 'reentrant'))
@pytest.mark.parametrize('route', HOST_ROUTES, ids=repr)
def test_a_checkpointed_layer_gives_the_plain_runs_gradients(route, reentrant):
    """(route 'crs' is LinearCRS on its PyTorch formulation: the one whose backward read ``ctx.saved_tensors`` twice)"""
    check_checkpointing(route, 'cpu', reentrant)


# ---- 4. no gradient, no sketch ----------------------------------------------------------------------------------------------------------
def watch(monkeypatch):
    """count the estimator products through the seams that exist for it -> Counter: 'project' (_native_project: every product on the kernels),
    'dense' (_native_sketch underneath it), 'gather' / 'scatter' (cabi_x.crs_gather / crs_scatter), 'sketch' (_sketch: every product of the
    PyTorch formulation of linear_grp) and 'randint' (torch.randint: the seed draws, _sampled_rows, the columns of the PyTorch LinearCRS)"""
    from fewbit_amd import cabi_x
    n = collections.Counter()

    def count(owner, name, key):
        real = getattr(owner, name)

        def counted(*args, **kwargs):
            n[key] += 1
            return real(*args, **kwargs)
        monkeypatch.setattr(owner, name, counted)

    count(linear, '_native_project', 'project')
    count(linear, '_native_sketch', 'dense')
    count(linear, '_sketch', 'sketch')
    count(cabi_x, 'crs_gather', 'gather')
    count(cabi_x, 'crs_scatter', 'scatter')
    count(torch, 'randint', 'randint')
    return n


def products(n):
    return n['project'] + n['gather'] + n['scatter'] + n['sketch']


def hooked(call):
    """-> (result of call(), [(shape, dtype) of every tensor offered to saved_tensors_hooks while it ran])"""
    seen = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (seen.append((tuple(t.shape), t.dtype)), t)[1], lambda t: t):
        out = call()
    return out, seen


def check_no_gradient_no_sketch(route, device, mode, monkeypatch):
    """grad mode off, or the weight frozen (input requiring grad, bias trainable): zero products, no tensor saved by a node of the layer's
    own, both generators untouched, the output -- and with the frozen weight input.grad and bias.grad -- bit-equal to F.linear's"""
    route.enter()
    gen = torch.Generator().manual_seed(5)
    layer = route.layer(device, generator=gen)
    x, w = route.data(device)
    xi = x.clone().requires_grad_()
    if mode == 'frozen weight':
        layer.weight.requires_grad_(False)
    n = watch(monkeypatch)
    before, gen_before = torch.get_rng_state(), gen.get_state()
    device_before = torch.cuda.get_rng_state(device) if torch.device(device).type == 'cuda' else None
    block = {'no_grad': torch.no_grad, 'inference_mode': torch.inference_mode, 'frozen weight': contextlib.nullcontext}[mode]
    with block():
        y, seen = hooked(lambda: layer(xi))
    assert products(n) == 0 and n['randint'] == 0 and n['dense'] == 0, (route, mode, dict(n))
    assert torch.equal(torch.get_rng_state(), before) and torch.equal(gen.get_state(), gen_before)
    assert device_before is None or torch.equal(torch.cuda.get_rng_state(device), device_before)
    xr = x.clone().requires_grad_()
    weight, bias = layer.weight.detach().clone(), layer.bias.detach().clone().requires_grad_()
    want, want_seen = hooked(lambda: F.linear(xr, weight, bias))
    assert y.shape == want.shape and y.dtype == want.dtype and torch.equal(y.detach(), want.detach())
    if mode != 'frozen weight':
        assert seen == [] and y.grad_fn is None and not y.requires_grad
        return
    assert seen == want_seen and type(y.grad_fn) is type(want.grad_fn), (route, seen, want_seen, y.grad_fn)
    (y * w).sum().backward()
    (want * w).sum().backward()
    assert layer.weight.grad is None and products(n) == 0 and n['randint'] == 0
    assert torch.equal(xi.grad, xr.grad) and torch.equal(layer.bias.grad, bias.grad)


@pytest.mark.parametrize('mode', ('no_grad', 'inference_mode', 'frozen weight'))
@pytest.mark.parametrize('route', HOST_ROUTES, ids=repr)
def test_no_gradient_no_sketch(route, mode, monkeypatch):
    check_no_gradient_no_sketch(route, 'cpu', mode, monkeypatch)


def check_products_of_a_checkpointed_step(route, device, monkeypatch, torch_crs=False):
    """re-entrant: the first pass runs under no_grad and launches nothing, the recomputation one forward product, backward one -- as a plain
    step.  Non-re-entrant recomputes under grad mode by design: its count is printed, not bounded.  (``torch_crs``: LinearCRS on its PyTorch
    formulation has no seam of its own; its one forward draw of columns is the ``torch.randint`` it makes, its backward makes none.)"""
    route.enter()
    layer = route.layer(device)
    x, w = route.data(device)
    n = watch(monkeypatch)
    counts = {}
    for name, forward in (('plain', None), ('re-entrant', lambda m, xi: checkpoint(m, xi, use_reentrant=True)),
                          ('non-re-entrant', lambda m, xi: checkpoint(m, xi, use_reentrant=False))):
        n.clear()
        step(layer, x, w, forward=forward)
        counts[name] = (n['randint'], 0) if torch_crs else (products(n), n['randint'])
    print(f'\n{route} on {device}: estimator products (and torch.randint calls) per step: {counts}')
    want = (1, 0) if torch_crs else (2, counts['plain'][1])
    assert counts['plain'] == want and counts['re-entrant'] == want, (route, counts)
    assert counts['non-re-entrant'][0] >= want[0]
    return counts


@pytest.mark.parametrize('route', HOST_ROUTES, ids=repr)
def test_a_reentrant_checkpointed_step_launches_one_forward_and_one_backward_product(route, monkeypatch):
    check_products_of_a_checkpointed_step(route, 'cpu', monkeypatch, torch_crs=route.kind == 'crs')


# ---- 5. edges of the batch --------------------------------------------------------------------------------------------------------------
def check_no_rows(route, device, shape):
    """``rows == 0``: nothing raises, y is F.linear's empty tensor, weight.grad is exactly zero with the weight's shape and dtype"""
    route.enter()
    layer = route.layer(device)
    x, w = route.data(device, shape=shape)
    y, (gw, gb, gx) = step(layer, x, w)
    assert y.shape == (*shape, route.fout) and y.dtype == layer.weight.dtype and y.device == x.device
    assert gw.shape == layer.weight.shape and gw.dtype == layer.weight.dtype and int(torch.count_nonzero(gw)) == 0
    assert gb.shape == layer.bias.shape and int(torch.count_nonzero(gb)) == 0 and gx.shape == x.shape


@pytest.mark.parametrize('shape', ((0, ), (2, 0)), ids=('0-rows', '2x0-rows'))
@pytest.mark.parametrize('route', HOST_ROUTES, ids=repr)
def test_an_empty_batch_gives_a_zero_weight_gradient(route, shape):
    check_no_rows(route, 'cpu', shape)


def check_one_row(route, device):
    """``rows == 1`` and ``proj_dim > rows``: the layer runs, y and input.grad are F.linear's, the gradients have their leaves' shapes"""
    route.enter()
    layer = route.layer(device)
    assert route.proj > 1
    x, w = route.data(device, shape=(1, ))
    y, (gw, gb, gx) = step(layer, x, w)
    assert torch.equal(y, F.linear(x, layer.weight, layer.bias).detach()) and torch.equal(gx, w @ layer.weight.detach())
    assert gw.shape == layer.weight.shape and gb.shape == layer.bias.shape and gx.shape == x.shape
    assert bool(torch.isfinite(gw).all()) and torch.equal(gb, w.reshape(-1, route.fout).sum(dim=0))


@pytest.mark.parametrize('route', HOST_ROUTES, ids=repr)
def test_a_single_row_with_a_larger_proj_dim(route):
    check_one_row(route, 'cpu')


def check_strided_grad_output(route, device):
    """a grad_output that is not unit-stride -- the expanded gradient of ``y.sum()``, a transposed ``gy`` -- gives the bits of its contiguous copy"""
    route.enter()
    layer = route.layer(device)
    x, _ = route.data(device)

    def run(backward):
        layer.zero_grad()
        xi = x.clone().requires_grad_()
        torch.manual_seed(RUN_SEED)
        backward(layer(xi))
        return grads(layer, xi)

    ones = run(lambda y: y.backward(torch.ones_like(y)))
    assert_same_bits(run(lambda y: y.sum().backward()), ones, f'{route}: the expanded gradient of y.sum()')
    g = torch.Generator().manual_seed(2)
    gy = torch.randn(route.fout, *route.shape, generator=g).to(device).movedim(0, -1)          # the features are the slowest dimension
    assert gy.shape == (*route.shape, route.fout) and not gy.is_contiguous() and gy.stride(-1) != 1
    assert_same_bits(run(lambda y: y.backward(gy)), run(lambda y: y.backward(gy.contiguous())), f'{route}: a transposed grad_output')


@pytest.mark.parametrize('route', HOST_ROUTES, ids=repr)
def test_a_grad_output_that_is_not_unit_stride(route):
    check_strided_grad_output(route, 'cpu')


def check_second_backward(route, device):
    """``retain_graph=True`` then a second backward: the same bits twice (backward regenerates the same S, rows or columns)"""
    route.enter()
    layer = route.layer(device)
    x, w = route.data(device)
    xi = x.clone().requires_grad_()
    torch.manual_seed(RUN_SEED)
    loss = (layer(xi) * w).sum()
    loss.backward(retain_graph=True)
    first = [t.clone() for t in grads(layer, xi)]
    layer.zero_grad()
    xi.grad = None
    loss.backward()
    assert int(torch.count_nonzero(first[0])) > 0
    assert_same_bits(grads(layer, xi), first, f'{route}: the second backward through a retained graph')


@pytest.mark.parametrize('route', HOST_ROUTES, ids=repr)
def test_a_second_backward_through_a_retained_graph_gives_the_same_bits(route):
    check_second_backward(route, 'cpu')


def check_one_layer_called_twice(route, device):
    """One layer on two inputs in one step: the second call draws another seed than the first, and weight.grad is the sum of the two single-call
    gradients for those seeds (a single run of the second call draws its seed after a first call that is thrown away)."""
    route.enter()
    layer = route.layer(device)
    (x1, w1), (x2, w2) = route.data(device, seed=1), route.data(device, seed=2)

    def run(calls, discard_first=False, seed=RUN_SEED):
        layer.zero_grad()
        torch.manual_seed(seed)
        if discard_first:
            layer(x1)
        sum((layer(x) * w).sum() for x, w in calls).backward()
        return layer.weight.grad.clone(), layer.bias.grad.clone()

    both = run([(x1, w1), (x2, w2)])
    first, second = run([(x1, w1)]), run([(x2, w2)], discard_first=True)
    second_on_first_seed = run([(x2, w2)])
    assert not torch.equal(second[0], second_on_first_seed[0]), f'{route}: the second call met the seed of the first'
    assert torch.equal(both[0], first[0] + second[0]) and torch.equal(both[1], first[1] + second[1]), route


@pytest.mark.parametrize('route', HOST_ROUTES, ids=repr)
def test_one_layer_called_twice_in_a_step_draws_two_seeds(route):
    check_one_layer_called_twice(route, 'cpu')


# ---- 6. an overflowed AMP step ----------------------------------------------------------------------------------------------------------
def check_overflow_stays_visible(route, device, amp=torch.bfloat16):
    """one inf in grad_output: weight.grad contains a non-finite value (what GradScaler skips a step on); nothing is flushed to zero"""
    route.enter()
    layer = route.layer(device)
    x, w = route.data(device)
    w.reshape(-1, route.fout)[5 % w.reshape(-1, route.fout).shape[0], 3] = float('inf')
    _, (gw, gb, gx) = step(layer, x, w, amp=amp)
    assert not bool(torch.isfinite(gw).all()), route
    assert not bool(torch.isfinite(gb[3])) and bool(torch.isfinite(gb[:3]).all())


@pytest.mark.parametrize('route', HOST_ROUTES, ids=repr)
def test_an_overflowed_gradient_stays_visible_in_the_weight_gradient(route):
    check_overflow_stays_visible(route, 'cpu')
