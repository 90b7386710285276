"""``VarianceEstimator`` the way a training script runs it: one wrapped layer called twice in a step, inside both modes of
``torch.utils.checkpoint``, ``no_grad`` / ``inference_mode`` evaluation between steps, a frozen weight, a 3-D input, a model that returns a tuple.

This file runs on host tensors, where ``gradient_moments`` is float64 PyTorch arithmetic: ``LinearGRP(8, 4, proj_dim=5)`` on 10 rows.  The
expectation is always ``variance.estimate_*`` on float64 copies of the operands of THAT call; the stored triple is float32 and is compared
to relative 1e-6, as tests/test_moments_host.py does.  tests/test_gpu_variance_training.py runs the ``check_*`` functions below on the
gfx950 kernels with the comparison and the bounds of tests/test_gpu_moments.py."""
import contextlib
import inspect

import pytest
import torch
from torch.utils.checkpoint import checkpoint

from fewbit_amd import variance
from fewbit_amd.linear import LinearGRP
from fewbit_amd.variance import GradientStorage, VarianceEstimator, catch_gradients

N_IN, N_OUT, PROJ, ROWS = 8, 4, 5, 10
REL = 1e-6


class HostKit:
    """what a check needs to know about where it runs: the layer, the operands, the comparison"""
    device, rows = 'cpu', ROWS

    def layer(self):
        torch.manual_seed(3)
        return LinearGRP(N_IN, N_OUT, proj_dim=PROJ)

    def bs_proj(self, rows):
        return PROJ

    def operands(self, rows, seed):
        """-> (x, w): the input and the fixed weights of the loss ``(y * w).sum()``, so the gradient that reaches the layer's output is ``w``"""
        g = torch.Generator().manual_seed(seed)
        shape = (rows, ) if isinstance(rows, int) else tuple(rows)
        return torch.randn(*shape, N_IN, generator=g), torch.randn(*shape, N_OUT, generator=g)

    def compare(self, got, x, g, bs, bs_proj, what):
        x, g = x.detach().reshape(-1, x.shape[-1]).double(), g.detach().reshape(-1, g.shape[-1]).double()
        want = (variance.estimate_correlation(x, g), variance.estimate_variance_sgd(x, g, bs), variance.estimate_variance_rmm(x, g, bs_proj))
        for name, a, b in zip(('corr', 'var_sgd', 'var_rmm'), got, want):
            assert a.dtype == torch.float32 and a.dim() == 0
            assert abs(float(a) - float(b)) <= REL * abs(float(b)), (what, name, float(a), float(b))


class Recorder:
    """an estimator around ``kit.layer()`` whose callback records (triple, step, the pair and the row counts the state holds at that moment)"""

    def __init__(self, kit, model=None):
        self.seen = []
        self.est = VarianceEstimator(kit.layer() if model is None else model, self.callback)

    def callback(self, corr, var_sgd, var_rmm, step):
        s = self.est.state
        self.seen.append(((corr, var_sgd, var_rmm), step, s.input, s.grad_output, s.bs, s.bs_proj))


def rows_of(t):
    return t.numel() // t.shape[-1]


# ---- 1. one layer called twice in a step ----------------------------------------------------------------------------------------------
def check_called_twice(kit, rows2):
    """two calls, one ``backward()``: two callbacks in backward order (the second call's first) with steps 0 and 1, each with the triple, the
    pair and the row counts of its OWN call"""
    rec = Recorder(kit)
    calls = [kit.operands(kit.rows, 1), kit.operands(rows2, 2)]
    sum((rec.est(x) * w).sum() for x, w in calls).backward()
    assert len(rec.seen) == 2 and [s[1] for s in rec.seen] == [0, 1] and rec.est.state.step == 2
    for (triple, step, x_seen, g_seen, bs, bs_proj), (x, w) in zip(rec.seen, reversed(calls)):
        what = f'called twice ({rows_of(calls[0][0])} and {rows_of(calls[1][0])} rows), callback {step}'
        assert x_seen.shape == x.shape and torch.equal(x_seen, x), what + ': the input of another call'
        assert torch.equal(g_seen, w.to(g_seen.dtype)), what + ': the gradient of another call'
        assert bs == rows_of(x) and bs_proj == kit.bs_proj(rows_of(x)), (what, bs, bs_proj)
        kit.compare(triple, x, g_seen, rows_of(x), kit.bs_proj(rows_of(x)), what)
    assert all(a is b for a, b in zip(rec.est.variance, rec.seen[-1][0]))
    return rec


@pytest.mark.parametrize('rows2', (10, 6))
def test_a_layer_called_twice_in_one_step_reports_each_calls_own_triple(rows2):
    check_called_twice(HostKit(), rows2)


# ---- 2. checkpointing -----------------------------------------------------------------------------------------------------------------
def check_checkpointed(kit, reentrant, rows=ROWS, amp=None):
    """``checkpoint(est, x)``: one callback per step with the plain run's triple (the same bits: the operands are the same), ``step`` advances
    by one per step -- the recomputation is no step"""
    rec = Recorder(kit)
    x, w = kit.operands(rows, 1)

    def run(forward):
        xi = x.clone().requires_grad_()
        ctx = torch.autocast(kit.device, dtype=amp) if amp is not None else contextlib.nullcontext()
        with ctx:
            y = forward(xi)
            loss = (y * w.to(y.dtype)).sum()
        loss.backward()
        return y

    run(rec.est)
    y = run(lambda xi: checkpoint(rec.est, xi, use_reentrant=reentrant))
    assert len(rec.seen) == 2 and [s[1] for s in rec.seen] == [0, 1] and rec.est.state.step == 2
    (plain, _, xp, gp, _, _), (ckpt, _, xc, gc, bs, bs_proj) = rec.seen
    assert torch.equal(xp, xc) and torch.equal(gp, gc) and torch.equal(xc, x) and torch.equal(gc, w.to(y.dtype))
    assert all(torch.equal(a, b) for a, b in zip(plain, ckpt)), (plain, ckpt)
    assert bs == rows_of(x) and bs_proj == kit.bs_proj(rows_of(x))
    kit.compare(ckpt, x, gc, bs, bs_proj, f'checkpoint(use_reentrant={reentrant})')
    return rec


@pytest.mark.parametrize('reentrant', (False, True), ids=('non-reentrant', 'reentrant'))
def test_a_checkpointed_estimator_reports_once_per_step(reentrant):
    check_checkpointed(HostKit(), reentrant)


# ---- 3. calls that cannot reach a backward --------------------------------------------------------------------------------------------
def count_copies(monkeypatch):
    """-> a dict counting ``GradientStorage.forward`` and ``Tensor.clone`` calls from here on"""
    n = {'forward': 0, 'clone': 0}
    real_forward, real_clone = GradientStorage.forward, torch.Tensor.clone

    def forward(self, input):
        n['forward'] += 1
        return real_forward(self, input)

    def clone(self, *args, **kwargs):
        n['clone'] += 1
        return real_clone(self, *args, **kwargs)

    monkeypatch.setattr(GradientStorage, 'forward', forward)
    monkeypatch.setattr(torch.Tensor, 'clone', clone)
    return n


def check_no_gradient_no_copy(kit, mode, monkeypatch, rows=ROWS, rows_eval=6):
    """after one real step: a call under ``no_grad`` / ``inference_mode`` / with nothing requiring grad copies nothing, returns the layer's output
    and leaves ``state.input``, ``.bs``, ``.bs_proj``, ``.variance`` and ``.step`` as that step left them; the next real step works"""
    rec = Recorder(kit)
    x, w = kit.operands(rows, 1)
    (rec.est(x) * w).sum().backward()
    state = rec.est.state
    held = (state.input, state.grad_output, state.variance, state.bs, state.bs_proj, state.step)
    assert torch.equal(state.input, x) and state.bs == rows_of(x) and state.step == 1
    xe, _ = kit.operands(rows_eval, 2)
    if mode == 'nothing requires grad':
        for p in rec.est.parameters():
            p.requires_grad_(False)
    with monkeypatch.context() as patch, {'no_grad': torch.no_grad, 'inference_mode': torch.inference_mode}.get(mode, contextlib.nullcontext)():
        n = count_copies(patch)
        y = rec.est(xe)
        want = rec.est.model(xe)
    assert n == {'forward': 0, 'clone': 0}, (mode, n)
    assert y.grad_fn is None and not y.requires_grad and y.shape == want.shape and torch.equal(y, want)
    now = (state.input, state.grad_output, state.variance, state.bs, state.bs_proj, state.step)
    assert all(a is b for a, b in zip(now[:3], held[:3])) and now[3:] == held[3:], (mode, now[3:], held[3:])
    for p in rec.est.parameters():
        p.requires_grad_(True)
    x2, w2 = kit.operands(rows, 3)
    (rec.est(x2) * w2).sum().backward()
    assert len(rec.seen) == 2 and rec.seen[1][1] == 1 and torch.equal(state.input, x2)
    kit.compare(rec.est.variance, x2, state.grad_output, rows_of(x2), kit.bs_proj(rows_of(x2)), f'the step after {mode}')
    return n


@pytest.mark.parametrize('mode', ('no_grad', 'inference_mode', 'nothing requires grad'))
def test_a_call_without_a_gradient_copies_nothing_and_leaves_the_state_alone(mode, monkeypatch):
    check_no_gradient_no_copy(HostKit(), mode, monkeypatch)


# ---- 4. what was true before stays true -----------------------------------------------------------------------------------------------
def test_after_a_backward_the_state_holds_that_backwards_pair_and_the_signatures_are_the_references():
    kit = HostKit()
    rec = Recorder(kit)
    x, w = kit.operands(ROWS, 1)
    xi = x.clone().requires_grad_()
    (rec.est(xi) * w).sum().backward()
    state = rec.est.state
    assert torch.equal(state.input, x) and state.input is not xi and state.input.data_ptr() != xi.data_ptr() and not state.input.requires_grad
    assert torch.equal(state.grad_output, w) and state.bs == ROWS and state.bs_proj == PROJ and state.step == 1
    kit.compare(rec.est.variance, x, w, ROWS, PROJ, 'one plain step')
    assert isinstance(state, GradientStorage)
    assert list(inspect.signature(GradientStorage.forward).parameters) == ['self', 'input']
    assert list(inspect.signature(GradientStorage.backward).parameters) == ['self', 'grad_output']
    assert list(inspect.signature(GradientStorage.postprocess).parameters) == ['self']
    assert list(inspect.signature(catch_gradients).parameters) == ['input', 'storage']
    assert list(inspect.signature(VarianceEstimator.__init__).parameters) == ['self', 'model', 'callback']
    # the two functions on a storage of the caller's own, as the reference uses them
    done = []

    class Mine(GradientStorage):
        def postprocess(self):
            done.append((self.input, self.grad_output))

    storage = Mine()
    storage.forward(xi)
    y = catch_gradients(xi * 2, storage)
    assert torch.equal(y, xi * 2)
    (y * w.new_ones(ROWS, N_IN) * 3).sum().backward()
    assert len(done) == 1 and torch.equal(done[0][0], x) and torch.equal(done[0][1], torch.full((ROWS, N_IN), 3.0))


def test_a_frozen_weight_with_an_input_that_requires_grad_still_reports():
    kit = HostKit()
    rec = Recorder(kit)
    rec.est.model.weight.requires_grad_(False)
    x, w = kit.operands(ROWS, 1)
    xi = x.clone().requires_grad_()
    (rec.est(xi) * w).sum().backward()
    assert len(rec.seen) == 1 and rec.seen[0][1] == 0 and rec.est.model.weight.grad is None and xi.grad is not None
    assert torch.equal(rec.est.state.input, x) and torch.equal(rec.est.state.grad_output, w)
    kit.compare(rec.est.variance, x, w, ROWS, PROJ, 'frozen weight')


def test_the_rows_of_a_3d_input_are_flattened():
    kit = HostKit()
    rec = Recorder(kit)
    x, w = kit.operands((2, 5), 1)
    (rec.est(x) * w).sum().backward()
    assert x.shape == (2, 5, N_IN) and len(rec.seen) == 1 and rec.est.state.bs == 10 and rec.est.state.bs_proj == PROJ
    assert rec.est.state.input.shape == x.shape and rec.est.state.grad_output.shape == w.shape
    kit.compare(rec.est.variance, x, w, 10, PROJ, '3-D input')


def test_the_first_element_of_a_tuple_returning_model_is_caught():
    kit = HostKit()

    class Pair(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.inner = kit.layer()

        def forward(self, x):
            return self.inner(x), 'aside', x.shape

    rec = Recorder(kit, Pair())
    x, w = kit.operands(ROWS, 1)
    out = rec.est(x)
    assert isinstance(out, tuple) and len(out) == 3 and out[1] == 'aside' and out[2] == x.shape
    (out[0] * w).sum().backward()
    assert len(rec.seen) == 1 and rec.est.state.bs == ROWS and rec.est.state.bs_proj == ROWS       # (no proj_dim attributes: B_proj = B)
    kit.compare(rec.est.variance, x, w, ROWS, ROWS, 'tuple-returning model')


def test_one_row_raises_the_zero_division_it_always_raised():
    kit = HostKit()
    rec = Recorder(kit)
    x, w = kit.operands(1, 1)
    y = rec.est(x)
    with pytest.raises(ZeroDivisionError):
        (y * w).sum().backward()
    assert rec.seen == [] and rec.est.state.step == 0
