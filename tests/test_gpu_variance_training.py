"""The checks of tests/test_variance_training.py on the gfx950 kernels (``cabi_x.row_moments`` / ``sum_squares`` and one GEMM): one wrapped layer
called twice with unequal row counts, both checkpoint modes, bf16 autocast with ``backward()`` after the block, ``no_grad`` between two steps.

The layer shapes are those of ``test_the_estimator_on_a_randomized_layer_matches_the_float64_formulas`` (tests/test_gpu_moments.py: 256 rows,
64 -> 96, ``proj_dim_ratio = 0.25``), and every triple is compared with that test's ``_check_triple``: the float64 formulas on the host on the
operands of the call the callback belongs to, within the bounds derived there."""
import collections

import pytest
import torch

import fewbit_amd as fewbit
from fewbit_amd import cabi_x, linear, variance
from test_gpu_moments import B, N_IN, N_OUT, NAME, _check_triple
from test_variance_training import Recorder, check_called_twice, check_checkpointed, check_no_gradient_no_copy

pytestmark = pytest.mark.gpu
DEV = 'cuda'
RATIO = 0.25


@pytest.fixture(autouse=True)
def kernels_on():
    prev = linear.use_native_sketch(True)
    yield
    linear.use_native_sketch(prev)


@pytest.fixture
def launches(monkeypatch):
    """calls of the two seams of a kernel-path postprocess: ``cabi_x.row_moments`` and ``variance._cross_product``"""
    n = collections.Counter()

    def count(owner, name):
        real = getattr(owner, name)

        def counted(*args, **kwargs):
            n[name] += 1
            return real(*args, **kwargs)
        monkeypatch.setattr(owner, name, counted)

    count(cabi_x, 'row_moments')
    count(cabi_x, 'sum_squares')
    count(variance, '_cross_product')
    return n


class GpuKit:
    device, rows = DEV, B

    def __init__(self, dtype, matmul='rademacher'):
        self.dtype, self.matmul = dtype, matmul

    def layer(self):
        torch.manual_seed(3)
        return fewbit.RandomizedLinear(N_IN, N_OUT, proj_dim_ratio=RATIO, matmul=self.matmul, device=DEV, dtype=self.dtype)

    def bs_proj(self, rows):
        return int(RATIO * rows)

    def operands(self, rows, seed):
        g = torch.Generator().manual_seed(seed)
        return torch.randn(rows, N_IN, generator=g).to(self.dtype).to(DEV), torch.randn(rows, N_OUT, generator=g).to(self.dtype).to(DEV)

    def compare(self, got, x, g, bs, bs_proj, what):
        assert 'fewbit_hipx_row_moments' in variance.variance_path(x, g)
        mixed = x.dtype != g.dtype                                    # (autocast: the GEMM multiplies in the narrower dtype)
        _check_triple(got, x, g, bs, bs_proj, False, f'{self.matmul} {NAME(self.dtype)} {what}', gemm_dtype=torch.bfloat16 if mixed else None)


@pytest.mark.parametrize('dtype', (torch.bfloat16, torch.float32), ids=NAME)
def test_a_layer_called_twice_with_unequal_row_counts_reports_each_calls_own_triple(dtype, launches):
    check_called_twice(GpuKit(dtype), 200)
    assert launches['row_moments'] == 2 and launches['_cross_product'] == 2 and launches['sum_squares'] == 2, dict(launches)


@pytest.mark.parametrize('reentrant', (False, True), ids=('non-reentrant', 'reentrant'))
@pytest.mark.parametrize('dtype,matmul', ((torch.bfloat16, 'rademacher'), (torch.float32, 'dct')), ids=('bf16-rademacher', 'fp32-dct'))
def test_a_checkpointed_estimator_reports_once_per_step(dtype, matmul, reentrant, launches):
    check_checkpointed(GpuKit(dtype, matmul), reentrant, rows=B)
    assert launches['row_moments'] == 2 and launches['_cross_product'] == 2, dict(launches)           # the plain step and the checkpointed one


@pytest.mark.parametrize('forward', ('plain', 'non-reentrant', 'reentrant'))
def test_bf16_autocast_with_backward_after_the_block(forward, launches):
    """an fp32 layer under bf16 autocast: the input stays fp32, the gradient is bf16, cross multiplies in bf16 (the mixed-dtype contract)"""
    kit = GpuKit(torch.float32)
    rec = check_checkpointed(kit, forward == 'reentrant', rows=B, amp=torch.bfloat16) if forward != 'plain' else None
    if rec is None:
        rec = Recorder(kit)
        x, w = kit.operands(B, 1)
        with torch.autocast('cuda', dtype=torch.bfloat16):
            y = rec.est(x)
            loss = (y * w.bfloat16()).sum()
        loss.backward()
        assert y.dtype == torch.bfloat16 and len(rec.seen) == 1
        kit.compare(rec.est.variance, x, w.bfloat16(), B, B // 4, 'autocast, backward() after the block')
    state = rec.est.state
    assert state.input.dtype == torch.float32 and state.grad_output.dtype == torch.bfloat16 and state.bs == B and state.bs_proj == B // 4
    assert launches['row_moments'] == launches['_cross_product'] == len(rec.seen)


@pytest.mark.parametrize('mode', ('no_grad', 'inference_mode', 'nothing requires grad'))
def test_a_call_without_a_gradient_between_two_steps_launches_and_copies_nothing(mode, launches, monkeypatch):
    check_no_gradient_no_copy(GpuKit(torch.bfloat16), mode, monkeypatch, rows=B, rows_eval=200)
    assert launches['row_moments'] == 2 and launches['_cross_product'] == 2 and launches['sum_squares'] == 2, dict(launches)     # the two real steps
