"""The loss of a row without a GPU (include/fewbit_hipx.h, "The loss of a row"; fewbit_amd/csrc/fewbit_xent.hip; fewbit_amd/xent.py): the three entry
points of the companion library (declared, exported, bound), the host evaluation -- the definition -- against ``torch.logsumexp``, ``F.cross_entropy``
and autograd in float64, the refusals of the two GPU entry points that are decided before anything is launched, and
``fewbit.functional.cross_entropy`` / ``fewbit.CrossEntropyLoss`` off the kernel path, where they are ``F.cross_entropy`` bit for bit."""
import re
import subprocess
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import fewbit
from fewbit_amd import cabi_x

ROOT = Path(__file__).resolve().parents[1]
SYMBOLS = ('fewbit_hipx_cross_entropy_host', 'fewbit_hipx_cross_entropy_forward', 'fewbit_hipx_cross_entropy_backward')
INF = float('inf')


# ---- the library: symbols, versions --------------------------------------------------------------------------------------------------------------
def test_the_three_symbols_are_declared_exported_and_bound_and_the_revision_is_still_2():
    header = (ROOT / 'include' / 'fewbit_hipx.h').read_text()
    declared = set(re.findall(r'\b(fewbit_hipx_\w+)\s*\(', header))
    out = subprocess.run(['nm', '-D', '--defined-only', str(cabi_x.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in SYMBOLS:
        assert name in declared and name in exported and name in cabi_x.SYMBOLS, name
    assert declared == set(cabi_x.SYMBOLS) == {name for name in exported if name.startswith('fewbit_hipx_')}
    assert cabi_x.lib().fewbit_hipx_revision() == cabi_x.REVISION == 2 and cabi_x.lib().fewbit_hipx_abi_version() == cabi_x.ABI_VERSION == 1
    assert re.search(r'#define FEWBIT_HIPX_ABI_VERSION 1\b', header) and re.search(r'#define FEWBIT_HIPX_REVISION 2\b', header)
    assert 'The loss of a row' in header and '_cross_entropy_forward, _cross_entropy_backward): inside revision 2' in header
    assert {'cross_entropy_host', 'cross_entropy_forward', 'cross_entropy_backward'} <= set(cabi_x.__all__)
    # the cap on the workgroups that the binding restates is the kernels'
    source = (ROOT / 'fewbit_amd' / 'csrc' / 'fewbit_xent.hip').read_text()
    assert cabi_x.CROSS_ENTROPY_MAX_GROUPS == int(re.search(r'constexpr size_t kMaxGroups = (\d+);', source).group(1))


def test_the_exports_exist_and_the_reference_list_of_modules_is_unchanged():
    assert fewbit.functional.cross_entropy is fewbit.xent.cross_entropy is fewbit.cross_entropy
    assert fewbit.CrossEntropyLoss is fewbit.xent.CrossEntropyLoss and issubclass(fewbit.CrossEntropyLoss, torch.nn.CrossEntropyLoss)
    assert 'CrossEntropyLoss' not in fewbit.modules.__all__ and 'cross_entropy' not in fewbit.modules.__all__
    # (the reference's list: one module per activation function of fewbit.functional and nothing else)
    assert len(fewbit.modules.__all__) == len(set(fewbit.modules.__all__)) == 22
    m = fewbit.CrossEntropyLoss.from_loss(torch.nn.CrossEntropyLoss(ignore_index=3, reduction='sum'), out_dtype=torch.float32, inplace_backward=True)
    assert (m.ignore_index, m.reduction, m.label_smoothing, m.weight, m.out_dtype, m.inplace_backward) == (3, 'sum', 0.0, None, torch.float32, True)
    assert 'gone' in fewbit.functional.cross_entropy.__doc__.lower() and 'second' in fewbit.functional.cross_entropy.__doc__


# ---- the host evaluation is the definition ------------------------------------------------------------------------------------------------------------
def draw(rows, width, salt=0):
    g = torch.Generator().manual_seed(17 + salt)
    x = (torch.rand(rows, width, generator=g) * 32 - 16).to(torch.float32)
    t = torch.randint(0, width, (rows, ), generator=g)
    grow = torch.randn(rows, generator=g, dtype=torch.float64)
    return x, t, grow


def torch64(x, t, grow, ignore_index=-100):
    xd = x.double().requires_grad_()
    loss = F.cross_entropy(xd, t, reduction='none', ignore_index=ignore_index)
    loss.backward(grow)
    return torch.logsumexp(x.double(), 1), loss.detach(), xd.grad


def close(got, want, rel=1e-12):
    """equal to ``rel`` relative (of the row's scale for a matrix), NaN where NaN, infinities equal"""
    assert got.shape == want.shape and torch.equal(torch.isnan(got), torch.isnan(want))
    finite = torch.isfinite(want)
    assert torch.equal(got[~finite & ~torch.isnan(want)], want[~finite & ~torch.isnan(want)])
    err = (got[finite] - want[finite]).abs()
    assert bool((err <= rel * want[finite].abs().clamp_min(1e-3)).all()), float(err.max())


@pytest.mark.parametrize('rows, width', ((1, 1), (3, 2), (5, 9), (4, 257), (2, 4099)))
def test_the_host_function_is_logsumexp_cross_entropy_and_its_gradient_in_float64(rows, width):
    x, t, grow = draw(rows, width, width)
    lse, loss, d = cabi_x.cross_entropy_host(x, t, grow=grow)
    want_lse, want_loss, want_d = torch64(x, t, grow)
    close(lse, want_lse)
    close(loss, want_loss)
    assert bool(((d - want_d).abs() <= 1e-12 * grow.abs()[:, None]).all())
    # without a gradient, and with grow = 1
    lse1, loss1, none = cabi_x.cross_entropy_host(x, t, want_grad=False)
    assert none is None and torch.equal(lse1, lse) and torch.equal(loss1, loss)
    _, _, d1 = cabi_x.cross_entropy_host(x, t)
    assert bool(((d1 - torch64(x, t, torch.ones(rows, dtype=torch.float64))[2]).abs() <= 1e-12).all())


@pytest.mark.parametrize('ignore_index', (-100, 3))
def test_ignored_rows_are_zero_and_still_have_their_lse(ignore_index):
    x, t, grow = draw(6, 11, 5)
    t[1] = t[4] = ignore_index
    lse, loss, d = cabi_x.cross_entropy_host(x, t, ignore_index, grow)
    want_lse, want_loss, want_d = torch64(x, t, grow, ignore_index)
    close(lse, want_lse)
    close(loss, want_loss)
    assert bool(((d - want_d).abs() <= 1e-12 * grow.abs()[:, None]).all())
    for r in (1, 4):
        assert loss[r] == 0 and not torch.signbit(loss[r]) and not d[r].any() and not torch.signbit(d[r]).any()


def test_minus_infinity_has_probability_zero_and_the_nan_rules_are_torchs():
    x, t, grow = draw(8, 13, 9)
    grow[0] = -2.0
    x[0, :5] = -INF                                             # some -inf, a negative grow: +0, not -0
    x[1, 1::2] = -INF                                           # alternating
    x[2] = -INF
    x[2, 7] = 1.5                                               # -inf everywhere but at one position (the target)
    t[0], t[1], t[2] = 7, 2, 7
    x[3] = -INF                                                 # -inf everywhere: NaN
    x[4, 3] = INF                                               # +inf: NaN
    x[5, 12] = float('nan')                                     # NaN: NaN
    x[6, 4] = -INF
    t[6] = 4                                                    # the target itself at -inf: loss +inf, finite gradients
    lse, loss, d = cabi_x.cross_entropy_host(x, t, grow=grow)
    want_lse, want_loss, want_d = torch64(x, t, grow)
    close(lse[[0, 1, 2, 6, 7]], want_lse[[0, 1, 2, 6, 7]])
    assert lse[3] == -INF and torch.isnan(lse[4]) and torch.isnan(lse[5])
    close(loss, want_loss)
    assert torch.isnan(loss[3:6]).all() and loss[6] == INF and loss[2] == 0
    assert torch.equal(torch.isnan(d), torch.isnan(want_d)) and torch.isnan(d[3:6]).all() and not torch.isnan(d[[0, 1, 2, 6, 7]]).any()
    rows = [0, 1, 2, 6, 7]
    assert bool(((d[rows] - want_d[rows]).abs() <= 1e-12 * grow.abs()[rows, None]).all())
    at = x[rows] == -INF
    at[3, 4] = False                                            # (row 6: the target's own place holds -grow)
    assert d[6, 4] == -grow[6]
    assert not d[rows][at].any() and not torch.signbit(d[rows][at]).any()


def test_the_host_function_refuses_what_the_launches_refuse():
    L = cabi_x.lib()
    x, t, out = torch.zeros(8), torch.zeros(1, dtype=torch.int64), torch.zeros(8, dtype=torch.float64)
    args = lambda **kw: [kw.get(k, v) for k, v in (('x', x.data_ptr()), ('t', t.data_ptr()), ('rows', 1), ('width', 8), ('ii', -100), ('g', None),
                                                   ('lse', out.data_ptr()), ('loss', out.data_ptr()), ('d', None))]
    assert L.fewbit_hipx_cross_entropy_host(*args()) == 0
    for kw, word in (({'rows': 0}, 'rows = 0'), ({'rows': 2**31 + 1}, 'rows'), ({'width': 0}, 'width = 0'), ({'width': 2**24 + 1}, 'width'),
                     ({'x': None}, 'null'), ({'t': None}, 'null'), ({'lse': None}, 'null'), ({'loss': None}, 'null'), ({'rows': 0, 'x': None}, 'rows = 0')):
        rc = L.fewbit_hipx_cross_entropy_host(*args(**kw))
        assert rc < 0 and word in L.fewbit_hipx_last_error().decode() and 'cross_entropy_host' in L.fewbit_hipx_last_error().decode(), kw


def test_a_target_out_of_range_is_nan_on_its_row_only():
    x, t, grow = draw(4, 7, 3)
    t[1], t[2] = 7, -1
    lse, loss, d = cabi_x.cross_entropy_host(x, t, grow=grow)
    close(lse, torch.logsumexp(x.double(), 1))
    assert torch.isnan(loss[1:3]).all() and torch.isnan(d[1:3]).all()
    keep = torch.tensor([0, 3])
    _, want_loss, want_d = torch64(x[keep], t[keep], grow[keep])
    close(loss[keep], want_loss)
    assert bool(((d[keep] - want_d).abs() <= 1e-12 * grow.abs()[keep, None]).all())


# ---- the refusals, before anything is launched (no device is touched: the pointers are never read) ---------------------------------------------------
P, Q, T, L, S, G = 0x10000, 0x80000, 0x20000, 0x30000, 0x40000, 0x50000     # addresses that are never dereferenced
BF16 = 2


def refused(rc, *words):
    message = cabi_x.lib().fewbit_hipx_last_error().decode()
    assert rc < 0 and all(word in message for word in words), (rc, message)


def test_the_forward_refuses():
    fwd = cabi_x.lib().fewbit_hipx_cross_entropy_forward
    refused(fwd(7, P, 3, 8, 8, T, -100, L, S, None), 'cross_entropy_forward', 'unknown dtype 7')
    refused(fwd(BF16, P, 0, 8, 8, T, -100, L, S, None), 'rows = 0')
    refused(fwd(BF16, P, 2**31 + 1, 8, 8, T, -100, L, S, None), 'rows = 2147483649')
    refused(fwd(BF16, P, 3, 0, 8, T, -100, L, S, None), 'width = 0')
    refused(fwd(BF16, P, 3, 2**24 + 1, 2**24 + 1, T, -100, L, S, None), 'width = 16777217')
    refused(fwd(BF16, P, 3, 8, 7, T, -100, L, S, None), 'ld = 7 < width = 8')
    for pointers in ((None, T, L, S), (P, None, L, S), (P, T, None, S), (P, T, L, None)):
        x, t, lse, loss = pointers
        refused(fwd(BF16, x, 3, 8, 8, t, -100, lse, loss, None), 'cross_entropy_forward', 'null pointer')


def test_the_backward_refuses():
    bwd = cabi_x.lib().fewbit_hipx_cross_entropy_backward
    refused(bwd(-1, P, 3, 8, 8, T, -100, L, G, 0, Q, 8, None), 'cross_entropy_backward', 'unknown dtype -1')
    refused(bwd(BF16, P, 0, 8, 8, T, -100, L, G, 0, Q, 8, None), 'rows = 0')
    refused(bwd(BF16, P, 3, 0, 8, T, -100, L, G, 0, Q, 8, None), 'width = 0')
    refused(bwd(BF16, P, 3, 8, 7, T, -100, L, G, 0, Q, 8, None), 'ld = 7 < width = 8')
    refused(bwd(BF16, P, 3, 8, 8, T, -100, L, G, 0, Q, 7, None), 'ld_out = 7 < width = 8')
    refused(bwd(BF16, P, 3, 8, 8, T, -100, L, G, 2, Q, 8, None), 'grow_stride = 2')
    for pointers in ((None, T, L, G, Q), (P, None, L, G, Q), (P, T, None, G, Q), (P, T, L, None, Q), (P, T, L, G, None)):
        x, t, lse, grow, out = pointers
        refused(bwd(BF16, x, 3, 8, 8, t, -100, lse, grow, 1, out, 8, None), 'cross_entropy_backward', 'null pointer')
    # an output that overlaps the logits without being the logits: shifted by one element, by a row, the last byte, another row stride
    for out, ld_out in ((P + 2, 8), (P + 16, 8), (P + 2 * (2 * 8 + 8) - 2, 8), (P - (2 * (2 * 8 + 8) - 2), 8), (P, 9)):
        refused(bwd(BF16, P, 3, 8, 8, T, -100, L, G, 1, out, ld_out, None), 'overlaps')
    # rows with gaps: the extent runs to the last element of the last row, not over its gap
    refused(bwd(BF16, P, 3, 8, 16, T, -100, L, G, 1, P + 2 * (2 * 16 + 8) - 2, 8, None), 'overlaps')


# ---- off the kernel path: F.cross_entropy, bit for bit ---------------------------------------------------------------------------------------------
def same(ours, theirs, x, *more):
    """the values and the gradients of ``ours(x)`` are those of ``theirs(x)`` to the bit"""
    a, b = x.clone().requires_grad_(), x.clone().requires_grad_()
    ya, yb = ours(a), theirs(b)
    assert ya.dtype == yb.dtype and ya.shape == yb.shape and torch.equal(ya, yb)
    g = torch.ones_like(ya) * 0.75
    ya.backward(g)
    yb.backward(g)
    assert torch.equal(a.grad, b.grad)


@pytest.mark.parametrize('reduction', ('mean', 'sum', 'none'))
def test_host_tensors_and_float64_are_torchs(reduction):
    x, t, _ = draw(7, 19)
    t[2] = -100
    for dtype in (torch.float32, torch.float64, torch.bfloat16):
        same(lambda v: fewbit.functional.cross_entropy(v, t, reduction=reduction), lambda v: F.cross_entropy(v, t, reduction=reduction), x.to(dtype))
        same(lambda v: fewbit.CrossEntropyLoss(reduction=reduction)(v, t), lambda v: F.cross_entropy(v, t, reduction=reduction), x.to(dtype))
    # the extra keywords are accepted and change nothing there
    same(lambda v: fewbit.functional.cross_entropy(v, t, reduction=reduction, out_dtype=torch.float64, inplace_backward=True),
         lambda v: F.cross_entropy(v, t, reduction=reduction), x)


def test_weights_label_smoothing_probability_targets_and_more_dimensions_are_torchs():
    x, t, _ = draw(7, 19, 1)
    w = torch.rand(19) + 0.5
    same(lambda v: fewbit.functional.cross_entropy(v, t, weight=w), lambda v: F.cross_entropy(v, t, weight=w), x)
    same(lambda v: fewbit.CrossEntropyLoss(weight=w)(v, t), lambda v: F.cross_entropy(v, t, weight=w), x)
    same(lambda v: fewbit.functional.cross_entropy(v, t, label_smoothing=0.1), lambda v: F.cross_entropy(v, t, label_smoothing=0.1), x)
    same(lambda v: fewbit.CrossEntropyLoss(label_smoothing=0.1, ignore_index=2)(v, t), lambda v: F.cross_entropy(v, t, label_smoothing=0.1, ignore_index=2), x)
    p = torch.softmax(torch.randn(7, 19), 1)
    same(lambda v: fewbit.functional.cross_entropy(v, p), lambda v: F.cross_entropy(v, p), x)
    x3 = torch.randn(2, 19, 5)
    t3 = torch.randint(0, 19, (2, 5))
    same(lambda v: fewbit.functional.cross_entropy(v, t3, reduction='sum'), lambda v: F.cross_entropy(v, t3, reduction='sum'), x3)
    same(lambda v: fewbit.functional.cross_entropy(v, t, None, None, -100, None, 'sum'), lambda v: F.cross_entropy(v, t, reduction='sum'), x)
    same(lambda v: fewbit.functional.cross_entropy(v[0], t[0]), lambda v: F.cross_entropy(v[0], t[0]), x)


def test_a_swapped_module_keeps_its_settings_and_computes_torchs_values_on_the_host():
    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.head, self.loss = torch.nn.Linear(8, 19), torch.nn.CrossEntropyLoss(ignore_index=1, reduction='sum')

        def forward(self, x, t):
            return self.loss(self.head(x), t)

    torch.manual_seed(3)
    model = Model()
    x, t = torch.randn(5, 8), torch.tensor([0, 1, 18, 4, 1])
    want = model(x, t)
    fewbit.map_module(model, lambda m, path: fewbit.CrossEntropyLoss.from_loss(m) if type(m) is torch.nn.CrossEntropyLoss else m)
    assert type(model.loss) is fewbit.CrossEntropyLoss and (model.loss.ignore_index, model.loss.reduction) == (1, 'sum')
    assert torch.equal(model(x, t), want)
