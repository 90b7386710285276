"""The checks of tests/test_dropout_training.py on the gfx950 kernel (``use_native_sketch(True)`` forced), at ``(3, 5, 43)``: 645 elements, 80 whole
blocks of eight and a tail of five -- plus what only the device has: a misaligned ``grad_output``, the device default generator inside a
checkpoint, an overflowed fp16 gradient, and the package's own sublayer captured into a graph.

Every reference is computed on the HOST: the mask from ``cabi_x.dropout_keep`` for the seed the call drew (recorded through
``linear._draw_seed``), the arithmetic by torch's host operators (``reference`` of tests/test_gpu_dropout.py), compared bit for bit, NaN by position."""
import pytest
import torch

import fewbit
from fewbit_amd import cabi, linear
from test_dropout_training import (RUN_SEED, SUB_P, SUB_SHAPE, Sublayer, block_data, check_autocast, check_checkpointed_block, check_in_place_on_a_view,
                                   check_in_place_without_grad_returns_the_input, check_one_module_called_twice, check_plain_block_is_the_definition,
                                   check_retained_graph, check_same_tensor_twice, check_strided_grad_output, check_sublayer, expected, keep_of,
                                   record_seeds)
from test_gpu_dropout import DEV, DTYPES, INT, assert_same, host_keep

pytestmark = pytest.mark.gpu
SHAPE, N = (3, 5, 43), 645
NAME = lambda d: str(d).split('.')[-1]                               # noqa: E731


@pytest.fixture(autouse=True)
def native_sketch_on():
    prev = linear.use_native_sketch(True)
    yield
    linear.use_native_sketch(prev)


@pytest.fixture
def seeds(monkeypatch):
    return record_seeds(monkeypatch)


# ---- 1. the host cases on the kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('inplace', (False, True), ids=('out-of-place', 'inplace'))
@pytest.mark.parametrize('reentrant', (False, True), ids=('non-reentrant', 'reentrant'))
def test_a_checkpointed_block_gives_the_plain_runs_bits(reentrant, inplace, seeds):
    check_plain_block_is_the_definition(DEV, seeds, inplace, shape=SHAPE)
    check_checkpointed_block(DEV, seeds, reentrant, inplace, shape=SHAPE)


@pytest.mark.parametrize('reentrant', (False, True), ids=('non-reentrant', 'reentrant'))
def test_a_checkpoint_with_the_device_default_generator_gives_the_plain_runs_bits(reentrant, seeds):
    """``checkpoint`` restores the default generators, the device's included: the recomputation draws the forward's seed from it"""
    gen = torch.cuda.default_generators[0]
    check_checkpointed_block(DEV, seeds, reentrant, False, generator=gen, shape=SHAPE)
    # (the seed came from the device generator: the host generator did not move during the step)
    torch.manual_seed(RUN_SEED)
    untouched = torch.get_rng_state()
    x = torch.ones(SHAPE, device=DEV)
    fewbit.functional.dropout(x, 0.5, generator=gen)
    assert torch.equal(torch.get_rng_state(), untouched)


@pytest.mark.parametrize('amp', (torch.bfloat16, torch.float16), ids=NAME)
def test_autocast_dtypes_and_backward_after_the_block(amp, seeds):
    check_autocast(DEV, seeds, amp, shape=SHAPE)
    check_plain_block_is_the_definition(DEV, seeds, amp=amp, shape=SHAPE)


@pytest.mark.parametrize('amp', (torch.bfloat16, torch.float16), ids=NAME)
@pytest.mark.parametrize('reentrant', (False, True), ids=('non-reentrant', 'reentrant'))
def test_a_checkpointed_block_under_autocast_with_backward_after_the_block(reentrant, amp, seeds):
    check_checkpointed_block(DEV, seeds, reentrant, False, amp=amp, backward_inside=False, shape=SHAPE)


@pytest.mark.parametrize('dtype', DTYPES, ids=NAME)
def test_one_module_called_twice_draws_two_seeds_and_two_masks(dtype, seeds):
    check_one_module_called_twice(DEV, seeds, dtype, SHAPE)


@pytest.mark.parametrize('dtype', DTYPES, ids=NAME)
def test_dropout_add_of_one_tensor_with_itself(dtype, seeds):
    check_same_tensor_twice(DEV, seeds, dtype, SHAPE)


def test_a_second_backward_through_a_retained_graph_gives_the_same_bits(seeds):
    check_retained_graph(DEV, seeds, SHAPE)


def test_a_grad_output_that_is_not_contiguous(seeds):
    check_strided_grad_output(DEV, seeds, SHAPE)


@pytest.mark.parametrize('dtype', DTYPES, ids=NAME)
def test_in_place_under_no_grad_returns_the_input_object_itself(dtype, seeds):
    check_in_place_without_grad_returns_the_input(DEV, seeds, dtype, SHAPE)


def test_in_place_on_a_view_of_a_non_leaf(seeds):
    check_in_place_on_a_view(DEV, seeds)


# ---- 2. what only the device has ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=NAME)
def test_a_misaligned_grad_output_gives_the_aligned_copys_bits(dtype, seeds):
    """forward on a 16-byte aligned tensor (the vector path); ``grad_output`` one element into its allocation (the element path)"""
    g = torch.Generator().manual_seed(31)
    x = torch.randn(SHAPE, generator=g).to(dtype).to(DEV).requires_grad_()
    gy = torch.randn(SHAPE, generator=g).to(dtype).to(DEV)
    buf = torch.full((N + 9, ), 77.0, dtype=dtype, device=DEV)
    shifted = buf[1:N + 1].view(SHAPE)
    shifted.copy_(gy)
    assert x.data_ptr() % 16 == 0 and gy.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == gy.element_size() and shifted.is_contiguous()
    y = fewbit.functional.dropout(x, 0.5)
    assert len(seeds) == 1
    (aligned, ) = torch.autograd.grad(y, x, gy, retain_graph=True)
    (misaligned, ) = torch.autograd.grad(y, x, shifted)
    want = expected(gy, None, seeds[0], 0.5)
    assert_same(aligned, want, f'{dtype} aligned grad_output')
    assert_same(misaligned, want, f'{dtype} misaligned grad_output')
    assert torch.equal(shifted, gy) and bool((buf[:1] == 77.0).all()) and bool((buf[N + 1:] == 77.0).all())


def test_an_inf_in_the_gradient_stays_inf_where_kept_and_is_zero_where_dropped(seeds):
    """fp16 autocast, an overflowed gradient: ``inf`` at a kept position stays ``inf`` (what GradScaler looks for), at a dropped one it is +0"""
    lin = torch.nn.Linear(43, 43).to(DEV)
    x = block_data(DEV, SHAPE)[0]
    with torch.autocast('cuda', dtype=torch.float16):
        h = lin(x)
        y = fewbit.functional.dropout(h, 0.5)
    assert h.dtype == torch.float16 and y.dtype == torch.float16 and len(seeds) == 1
    keep = keep_of(seeds[0], SHAPE, 0.5).flatten()
    kept, dropped = int(keep.nonzero()[0]), int((~keep).nonzero()[0])
    gy = torch.randn(N, generator=torch.Generator().manual_seed(32)).half()
    gy[kept] = gy[dropped] = float('inf')
    (gh, ) = torch.autograd.grad(y, h, gy.view(SHAPE).to(DEV))
    assert_same(gh, expected(gy.view(SHAPE), None, seeds[0], 0.5), 'an inf in the gradient')
    flat = gh.flatten().cpu()
    assert float(flat[kept]) == float('inf') and int(flat.view(torch.int16)[dropped]) == 0


# ---- 3. a whole sublayer of this package --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('amp', (None, torch.bfloat16), ids=('plain', 'bf16-autocast'))
def test_a_sublayer_of_this_package_checkpointed_with_backward_after_the_autocast_block(amp, seeds):
    check_sublayer(DEV, seeds, amp, draws=3, saved_bytes=amp is None)


def test_the_sublayer_captured_into_a_graph_draws_fresh_masks_on_every_replay(monkeypatch):
    """one eager step on a side stream, the capture, three replays.  The step exposes both dropouts: ``d1 = drop(h)`` and
    ``y = dropout_add(d1, x)``, with the gradients that reach ``h`` and ``d1`` (``gy`` has no zero, so the gradient of ``d1`` is zero exactly where
    the second dropout dropped, and the gradient of ``h`` where either did).  Each pattern is the host mask of the seed the replay counter gave
    that call: the counter is read by the layer, the first and the second dropout in this order."""
    m = Sublayer().to(DEV)
    n = 2 * 19 * 24
    x = block_data(DEV, SUB_SHAPE)[0]
    gy = torch.rand(SUB_SHAPE, generator=torch.Generator().manual_seed(33)).to(DEV) + 0.5

    def step():
        h = m.fc2(m.act(m.fc1(x)))
        d1 = m.drop(h)
        y = fewbit.functional.dropout_add(d1, x, SUB_P)
        g_h, g_d1, g_w = torch.autograd.grad(y, [h, d1, m.fc1.model.weight], gy)
        return h, d1, y, g_h, g_d1, g_w

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                        # the eager warm-up: the per-device replay counter exists from here on
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    bases = []
    monkeypatch.setattr(linear, '_draw_seed', lambda generator: bases.append(0x1234567 + 77 * len(bases)) or bases[-1])
    counter = linear._replay_counter(torch.device(DEV))
    c0 = int(counter)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        h, d1, y, g_h, g_d1, g_w = step()
    assert len(bases) == 3 and int(counter) == c0
    threshold, first, second = 6554, [], []
    for replay in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert int(counter) == c0 + 3 * (replay + 1)                  # the same amount per replay: one word per seeded call
        assert bool((h != 0).all()) and bool(torch.isfinite(g_w).all()) and int(torch.count_nonzero(g_w)) > 0
        dropped1, dropped2 = (d1 == 0), (g_d1 == 0)
        keep1 = host_keep(cabi.mix_sketch_seed(bases[1], c0 + 3 * replay + 1), n, threshold).view(SUB_SHAPE)
        keep2 = host_keep(cabi.mix_sketch_seed(bases[2], c0 + 3 * replay + 2), n, threshold).view(SUB_SHAPE)
        assert torch.equal(~dropped1.cpu(), keep1) and torch.equal(~dropped2.cpu(), keep2)
        # each backward met its own forward's mask
        assert torch.equal(g_h == 0, dropped1 | dropped2)
        assert torch.equal((y == x)[d1 != 0], dropped2[d1 != 0]) and torch.equal(y[dropped2].view(INT[y.dtype]), x[dropped2].view(INT[x.dtype]))
        assert_same(d1, expected(h, None, cabi.mix_sketch_seed(bases[1], c0 + 3 * replay + 1), SUB_P), f'replay {replay}: the first dropout')
        assert_same(y, expected(d1, x, cabi.mix_sketch_seed(bases[2], c0 + 3 * replay + 2), SUB_P), f'replay {replay}: the second dropout')
        assert not torch.equal(dropped1, dropped2)
        first.append(dropped1.clone())
        second.append(dropped2.clone())
    for drops in (first, second):
        assert not torch.equal(drops[0], drops[1]) and not torch.equal(drops[1], drops[2]) and not torch.equal(drops[0], drops[2])
