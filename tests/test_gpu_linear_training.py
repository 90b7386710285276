"""The checks of tests/test_linear_training.py on the gfx950 kernels (``use_native_sketch(True)`` forced): LinearGRP / LinearCRS under autocast
with ``backward()`` inside and after the block, under both checkpoint modes, under ``no_grad`` / ``inference_mode`` / a frozen weight and at
the edges of a batch -- plus the one check that needs the kernels' own definitions: the autocast weight gradient against a float64
expectation built from what the host evaluates for the pinned seed (tests/sketch_reference.py, ``cabi.sampled_rows``, ``cabi_x.crs_columns``).

The shapes are the smallest at which each route still takes its kernel.  Nothing loops over draws."""
import pytest
import torch

from fewbit_amd import cabi, cabi_x, linear
from test_linear_training import (Route, check_backward_outside_autocast, check_checkpointing, check_no_gradient_no_sketch, check_no_rows,
                                  check_one_layer_called_twice, check_one_row, check_overflow_stays_visible,
                                  check_products_of_a_checkpointed_step, check_second_backward, check_strided_grad_output, step, watch)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32

ROUTES = [
    Route('rademacher', 'rademacher', (3, 200), 72, 40, 96),            # the shape of test_layer_through_the_native_sketch_... (3-D input)
    Route('gaussian', 'gaussian', (3, 200), 72, 40, 96),
    Route('dct', 'dct', (256, ), 72, 40, 64),                           # 256 rows: the smallest row count with a kernel pair
    Route('dft', 'dft', (256, ), 72, 40, 64),
    Route('dct-zext', 'dct', (200, ), 72, 40, 64, extend=True),         # use_row_extension(True): zero-extended to N' = 256
    Route('crs', 'crs', (256, ), 72, 40, 36),
]
DFT_ZEXT = Route('dft-zext', 'dft', (200, ), 72, 40, 64, extend=True)
BY_NAME = {r.name: r for r in ROUTES}


@pytest.fixture(autouse=True)
def kernels_on_and_switches_restored():
    """these tests are about the kernels: select them whatever the environment says; a route sets the row-extension switch it needs"""
    native, extend = linear.use_native_sketch(True), linear.use_row_extension()
    yield
    linear.use_native_sketch(native)
    linear.use_row_extension(extend)


def on_the_kernels(n):
    """products the counters of ``watch`` saw on the kernels (every linear_grp product goes through _native_project, LinearCRS's two calls
    through cabi_x)"""
    return n['project'] + n['gather'] + n['scatter']


def test_every_route_is_the_one_its_name_says():
    """the path texts and predicates the layer decides by, at the shapes of ROUTES: a later change of route shows up here by name"""
    for route in ROUTES + [DFT_ZEXT]:
        route.enter()
        layer = route.layer(DEV)
        x, _ = route.data(DEV)
        flat = x.reshape(-1, route.fin)
        if route.kind == 'crs':
            assert linear._native_crs_applies(flat, layer.weight, route.proj)
            # bf16 activations with an fp32 master weight (an inner layer under autocast): the PyTorch formulation, by _native_crs_applies
            assert not linear._native_crs_applies(flat.to(BF16), layer.weight, route.proj)
        elif route.kind in ('gaussian', 'rademacher'):
            assert linear._native_sketch_applies(route.kind, flat, None) and linear._native_sketch_applies(route.kind, flat.to(BF16), None)
        else:
            path = linear.sampled_transform_path(route.kind, flat)
            assert (f'fewbit_hipx_sampled_{route.kind}_zext' in path and 'zero-extended to 256 rows' in path) if route.extend else \
                ('kernel pair fewbit_hip' in path and 'zext' not in path), (route, path)
            assert linear._native_transform_rows(route.kind, flat) == 256


# ---- 1. backward() after the autocast block ---------------------------------------------------------------------------------------------
AMP_CASES = [(r, BF16, d) for r in ROUTES for d in (FP32, BF16)] + [(BY_NAME[k], FP16, d) for k in ('rademacher', 'dct') for d in (FP32, FP16)]


@pytest.mark.parametrize('route,amp,in_dtype', AMP_CASES, ids=lambda v: str(v).replace('torch.', ''))
def test_backward_after_the_autocast_block_equals_backward_inside_it(route, amp, in_dtype, monkeypatch):
    n = watch(monkeypatch)
    check_backward_outside_autocast(route, DEV, in_dtype, amp)
    if route.kind == 'crs' and in_dtype != FP32:
        assert on_the_kernels(n) == 0 and n['randint'] == 2          # LinearCRS, 16-bit input and fp32 weight: the PyTorch formulation
    else:
        assert on_the_kernels(n) == 4 and n['sketch'] == 0, dict(n)     # two steps on the kernels: a forward and a backward product each


# ---- 2. the autocast gradient is the estimator's ----------------------------------------------------------------------------------------
SEED = 0x5eed5eed5eed


def expected_weight_gradient(route, seed, x, gy, in_dtype, amp):
    """float64 ``(S G)^T (S X)`` for the S, rows or columns of ``seed``, with the roundings the docstring of fewbit_amd/linear.py states: the
    operands of the dense matrix pipe are bf16; the kept projection has the dtype of the input; the projection of the gradient has the
    gradient's dtype (the autocast dtype); both meet in a GEMM of the autocast dtype, so the kept projection is rounded to it once more.
    The rounding of that GEMM's result is not modelled: it is what the tolerance is for."""
    import sketch_reference as ref
    fin, p = route.fin, route.proj
    flat, g = x.reshape(-1, fin).cpu(), gy.reshape(-1, route.fout).cpu().double()
    rows = flat.shape[0]

    def kept(t):
        return t.to(in_dtype).to(amp).double()

    def grad(t):
        return t.to(amp).double()

    if route.kind in ('gaussian', 'rademacher'):
        sx = ref.matrix(route.kind, seed, p, rows, in_dtype).double() @ flat.to(BF16).double() / p
        sg = ref.matrix(route.kind, seed, p, rows, amp).double() @ g
        return grad(sg).T @ kept(sx)
    if route.kind == 'crs':
        cols, count = cabi_x.crs_columns(seed, fin, p)
        scale = (count.double() * fin / p).float()
        want = torch.zeros(route.fout, fin, dtype=torch.float64)
        want[:, cols] = g.T @ kept(flat.float()[:, cols] * scale)
        return want
    big = 256
    k = cabi.sampled_rows(seed, big, p)
    xp, gp = torch.zeros(big, fin, dtype=torch.float64), torch.zeros(big, route.fout, dtype=torch.float64)
    xp[:rows], gp[:rows] = flat.double(), g
    if route.kind == 'dct':
        return grad(linear.dct(gp, dim=0, norm='ortho')[k]).T @ kept(linear.dct(xp, dim=0, norm='ortho')[k] * (big / p))
    sx, sg = torch.fft.fft(xp, dim=0, norm='ortho')[k] * (big / p), torch.fft.fft(gp, dim=0, norm='ortho')[k]
    return grad(sg.real).T @ kept(sx.real) + grad(sg.imag).T @ kept(sx.imag)


# The tolerance of the plain-layer test of each route whose final GEMM has the autocast dtype, bf16, as a fraction of max|want|:
# test_layer_through_the_native_sketch_... (bf16: 3e-2), the layer tests of test_gpu_dct.py, test_gpu_dft.py and test_gpu_transform_zext.py
# (bf16: 3e-2).  'dft' adds its two planes in a second bf16 GEMM (addmm): one more bf16 rounding of a p-term sum, 2^-8 of a value no larger
# than the sum of the two plane products -- inside 3e-2, no allowance is added.
# LinearCRS: tests/test_gpu_crs.py has an fp32 layer test only (2e-4: two fp32 GEMMs in another summation order).  Under autocast G^T kept is
# a bf16 GEMM: fp32 sums of exact products of bf16 operands, rounded ONCE to bf16 -- bf16 carries 8 significant bits, so one rounding to
# nearest moves an entry by at most 2^-8 of itself (tests/test_gpu_crs_edges.py: U_OUT), at most 2^-8 of max|want|.  That one rounding is
# added to the existing figure and nothing else is.
TOLERANCE = {'rademacher': 3e-2, 'gaussian': 3e-2, 'dct': 3e-2, 'dft': 3e-2, 'dct-zext': 3e-2, 'crs': 2e-4 + 2.0**-8}
ESTIMATOR_CASES = [(r, d) for r in ROUTES for d in (FP32, BF16) if not (r.kind == 'crs' and d == BF16)]     # (crs, bf16 input: the PyTorch formulation)


@pytest.mark.parametrize('route,in_dtype', ESTIMATOR_CASES, ids=lambda v: str(v).replace('torch.', ''))
def test_the_autocast_weight_gradient_is_the_estimators(route, in_dtype, monkeypatch):
    """an fp32 layer under bf16 autocast, ``backward()`` after the block, the seed pinned: weight.grad against the float64 expectation"""
    monkeypatch.setattr(linear, '_draw_seed', lambda generator: SEED)
    route.enter()
    layer = route.layer(DEV)
    x, w = route.data(DEV, in_dtype)
    n = watch(monkeypatch)
    _, (gw, gb, gx) = step(layer, x, w, amp=BF16, backward_inside=False)
    assert on_the_kernels(n) == 2 and n['sketch'] == 0 and gw.dtype == FP32
    want = expected_weight_gradient(route, SEED, x, w.to(BF16), in_dtype, BF16)
    top = float(want.abs().max())
    err = float((gw.cpu().double() - want).abs().max()) / top
    print(f'\nautocast bf16, {route}, {str(in_dtype)[6:]} input: error / tolerance = {err:.3g} / {TOLERANCE[route.name]:.3g} = {err / TOLERANCE[route.name]:.3f}')
    assert top > 0 and err <= TOLERANCE[route.name], (route, in_dtype, err)
    if route.kind == 'crs':                                            # outside the drawn columns: exactly +0
        rest = torch.ones(route.fin, dtype=torch.bool)
        rest[cabi_x.crs_columns(SEED, route.fin, route.proj)[0]] = False
        assert not bool(gw.cpu()[:, rest].view(torch.int32).any())


# ---- 3. checkpointing -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reentrant', (False, True), ids=('non-reentrant', 'reentrant'))
@pytest.mark.parametrize('route', ROUTES, ids=repr)
def test_a_checkpointed_layer_gives_the_plain_runs_gradients(route, reentrant, monkeypatch):
    n = watch(monkeypatch)
    check_checkpointing(route, DEV, reentrant)
    assert on_the_kernels(n) >= 4 and n['sketch'] == 0, dict(n)


def test_linear_crs_with_bf16_input_and_fp32_weight_under_autocast_and_a_non_reentrant_checkpoint(monkeypatch):
    """bf16 activations, fp32 master weight: ``_native_crs_applies`` wants equal dtypes, so this is LinearCRS on its PyTorch formulation (randint
    + bincount + nonzero) on the GPU -- the route whose backward read ``ctx.saved_tensors`` twice.  Stated by name: if a later change moves this
    dtype combination onto the kernels, the counters below say so."""
    route = BY_NAME['crs']
    n = watch(monkeypatch)
    check_checkpointing(route, DEV, False, amp=BF16, in_dtype=BF16)
    assert n['gather'] == 0 and n['scatter'] == 0 and n['randint'] == 3, dict(n)       # a plain step, the checkpointed forward, its recomputation


# ---- 4. no gradient, no sketch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ('no_grad', 'inference_mode', 'frozen weight'))
@pytest.mark.parametrize('route', ROUTES, ids=repr)
def test_no_gradient_no_sketch(route, mode, monkeypatch):
    check_no_gradient_no_sketch(route, DEV, mode, monkeypatch)


@pytest.mark.parametrize('route', ROUTES, ids=repr)
def test_a_reentrant_checkpointed_step_launches_one_forward_and_one_backward_product(route, monkeypatch):
    route.enter()
    n = watch(monkeypatch)
    step(route.layer(DEV), *route.data(DEV))
    assert on_the_kernels(n) == 2 and n['dense'] == (2 if route.kind in ('gaussian', 'rademacher') else 0), dict(n)
    monkeypatch.undo()
    check_products_of_a_checkpointed_step(route, DEV, monkeypatch)


# ---- 5. edges of the batch --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', ((0, ), (2, 0)), ids=('0-rows', '2x0-rows'))
@pytest.mark.parametrize('route', ROUTES + [DFT_ZEXT], ids=repr)
def test_an_empty_batch_gives_a_zero_weight_gradient(route, shape, monkeypatch):
    n = watch(monkeypatch)
    check_no_rows(route, DEV, shape)
    assert on_the_kernels(n) == 0 and n['sketch'] == 0 and n['randint'] == 0, dict(n)      # no kernel call with rows = 0, no randint(0, 0)


@pytest.mark.parametrize('route', ROUTES + [DFT_ZEXT], ids=repr)
def test_a_single_row_with_a_larger_proj_dim(route):
    check_one_row(route, DEV)


@pytest.mark.parametrize('route', ROUTES, ids=repr)
def test_a_grad_output_that_is_not_unit_stride(route):
    check_strided_grad_output(route, DEV)


@pytest.mark.parametrize('route', ROUTES, ids=repr)
def test_a_second_backward_through_a_retained_graph_gives_the_same_bits(route):
    check_second_backward(route, DEV)


@pytest.mark.parametrize('route', ROUTES, ids=repr)
def test_one_layer_called_twice_in_a_step_draws_two_seeds(route, monkeypatch):
    seeds, draw = [], linear._draw_seed
    monkeypatch.setattr(linear, '_draw_seed', lambda generator: (seeds.append(draw(generator)), seeds[-1])[1])
    check_one_layer_called_twice(route, DEV)
    assert len(seeds) >= 2 and seeds[0] != seeds[1]                 # the first run of the check: two calls in one step


# ---- 6. an overflowed AMP step ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('amp', (BF16, FP16), ids=('bf16', 'fp16'))
@pytest.mark.parametrize('route', ROUTES, ids=repr)
def test_an_overflowed_gradient_stays_visible_in_the_weight_gradient(route, amp):
    check_overflow_stays_visible(route, DEV, amp)
