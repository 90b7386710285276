"""``fewbit_hipx_glu_backward_product`` on the GPU through its binding (fewbit_amd/csrc/fewbit_glu.hip, the PRODUCT kernels): ``d_gate`` and ``d_up`` byte
for byte those of ``glu_backward`` on the same state; ``product = act(g^) u^`` byte for byte the forward's own ``y`` on the decodes (fp32) and within
the forward's bound of float64 (16-bit); guards, row gaps, ``gy`` and the state untouched; every subset of the three outputs; poisoned groups;
refusals.  Sizes: where the plan changes (one row of 1 .. 65), the halves of a 144-column buffer, blocks that straddle rows, a base one element
off, one second sweep."""
import itertools

import pytest
import torch

from fewbit_amd import cabi, cabi_x
from gated_mlp_harness import Strided, inputs, same_bytes, within_16_bit_bound
from glu_harness import act64, decoded
from norm_harness import DEV, Guarded

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.float16, torch.bfloat16)
BITS = (2, 4, 8)
ACTIVATIONS = ('silu', 'gelu')
SEED = 0x0123456789abcdef


def combinations():
    return [(dtype, bits, activation) for dtype in DTYPES for bits in BITS for activation in ACTIVATIONS]


def check_product(product, host_state, rows, width, bits, activation, dtype, label):
    """fp32: the bytes of the forward on the uploaded decodes; 16-bit: the forward's bound against float64"""
    gq, uq = (t.view(rows, width) for t in decoded(host_state, rows * width, bits))
    if dtype == torch.float32:
        y, _ = cabi_x.glu_forward(gq.to(DEV), uq.to(DEV), activation, keep=False)
        assert same_bytes(product, y), label
    else:
        exact = act64(gq, activation) * uq.double()
        assert bool(within_16_bit_bound(product.cpu(), exact, dtype).all()), label


def run(rows, width, ld_gate, ld_up, ld_product, off, dtype, bits, activation, salt=0):
    """one forward for the state, then the old backward into dense tensors and the new one into guarded, strided buffers"""
    label = f'{rows}x{width} ld {ld_gate}/{ld_up}/{ld_product} off {off} {dtype} bits {bits} {activation}'
    n = rows * width
    gate, up, gy = inputs(rows, width, dtype, salt)
    _, state = cabi_x.glu_forward(gate.to(DEV), up.to(DEV), activation, bits, SEED)
    host = cabi_x.glu_state_host(gate.float(), up.float(), SEED, bits)
    assert torch.equal(state.cpu(), host), label
    S = Guarded(state.numel(), torch.uint8, like=state)
    GY = Guarded(n, dtype, off, like=gy.to(DEV))
    old_gate, old_up = cabi_x.glu_backward(gy.to(DEV), state, activation, bits)
    DG, DU, PR = Strided(rows, width, ld_gate, dtype, off), Strided(rows, width, ld_up, dtype, off), Strided(rows, width, ld_product, dtype, off)
    d_gate, d_up, product = cabi_x.glu_backward_product(GY.t.view(rows, width), S.t, activation, bits, d_gate=DG.view, d_up=DU.view, product=PR.view)
    torch.cuda.synchronize()
    assert DG.only_the_matrix_was_written() and DU.only_the_matrix_was_written() and PR.only_the_matrix_was_written(), label
    assert GY.unchanged() and S.unchanged(), label
    assert same_bytes(d_gate, old_gate) and same_bytes(d_up, old_up), label
    check_product(product, host, rows, width, bits, activation, dtype, label)
    return d_gate.clone(), d_up.clone(), product.clone()


# ---- sizes and layouts ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', (1, 7, 8, 9, 63, 64, 65))
def test_one_row(n):
    for dtype, bits, activation in combinations():
        run(1, n, n, n, n, 0, dtype, bits, activation)


def test_the_halves_of_a_matrix_of_144_columns_and_the_product_in_a_third_buffer():
    """[d_gate | d_up] in ONE 3 x 144 buffer, as the node of the gated MLP lays them out: the vector path steps over the other half"""
    rows, width = 3, 72
    for dtype, bits, activation in combinations():
        gate, up, gy = inputs(rows, width, dtype)
        _, state = cabi_x.glu_forward(gate.to(DEV), up.to(DEV), activation, bits, SEED)
        old_gate, old_up = cabi_x.glu_backward(gy.to(DEV), state, activation, bits)
        both, PR = Guarded(rows * 2 * width, dtype), Guarded(rows * width, dtype)
        matrix = both.t.view(rows, 2 * width)
        d_gate, d_up, product = cabi_x.glu_backward_product(gy.to(DEV), state, activation, bits, d_gate=matrix[:, :width], d_up=matrix[:, width:],
                                                            product=PR.t.view(rows, width))
        torch.cuda.synchronize()
        assert both.intact() and PR.intact()
        assert same_bytes(matrix, torch.cat((old_gate, old_up), dim=1))
        check_product(product, state.cpu(), rows, width, bits, activation, dtype, f'{dtype} {bits} {activation}')
        dense = run(rows, width, width, width, width, 0, dtype, bits, activation)
        assert same_bytes(d_gate, dense[0]) and same_bytes(d_up, dense[1]) and same_bytes(product, dense[2])


def test_blocks_that_straddle_rows_take_the_element_path():
    for dtype, bits, activation in combinations():
        run(2, 100, 100, 100, 100, 0, dtype, bits, activation)
        run(2, 100, 100, 104, 108, 0, dtype, bits, activation, salt=1)


def test_a_base_one_element_off_or_an_odd_stride_takes_the_element_path_with_the_same_bytes():
    for dtype, bits, activation in combinations():
        aligned = run(3, 24, 24, 24, 24, 0, dtype, bits, activation)
        shifted = run(3, 24, 24, 24, 24, 1, dtype, bits, activation)
        gaps = run(3, 24, 40, 32, 48, 1, dtype, bits, activation)
        odd = run(3, 24, 24, 24, 25, 0, dtype, bits, activation)           # the product's stride alone misses the 16-byte rule
        for other in (shifted, gaps, odd):
            assert all(same_bytes(a, b) for a, b in zip(aligned, other))


def test_a_lane_takes_a_second_sweep():
    n = cabi_x.QUANT_SWEEP + 11
    run(1, n, n, n, n, 0, torch.bfloat16, 4, 'silu')


# ---- every subset of the three outputs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_every_subset_of_the_outputs_has_the_bytes_of_the_full_call(dtype):
    rows, width = 5, 72
    for bits, activation in itertools.product(BITS, ACTIVATIONS):
        gate, up, gy = inputs(rows, width, dtype, 3)
        gyd = gy.to(DEV)
        _, state = cabi_x.glu_forward(gate.to(DEV), up.to(DEV), activation, bits, SEED)
        full = cabi_x.glu_backward_product(gyd, state, activation, bits)
        for want in itertools.product((False, True), repeat=3):
            buffers = [Guarded(rows * width, dtype) for _ in range(3)]
            views = [b.t.view(rows, width) for b in buffers]
            outs = cabi_x.glu_backward_product(gyd, state, activation, bits, want, *views)
            torch.cuda.synchronize()
            for got, whole, wanted, buffer in zip(outs, full, want, buffers):
                assert (got is None) != wanted and buffer.intact()
                assert same_bytes(got, whole) if wanted else buffer.unchanged(), (dtype, bits, activation, want)
        # no gy: the product alone
        P = Guarded(rows * width, dtype)
        none_gate, none_up, product = cabi_x.glu_backward_product(None, state, activation, bits, (False, False, True), product=P.t.view(rows, width))
        torch.cuda.synchronize()
        assert none_gate is None and none_up is None and P.intact() and same_bytes(product, full[2])
        # through the entry point itself: NULL outputs next to a guarded one; all three NULL: no launch
        D = Guarded(rows * width, dtype)
        f, stream = cabi_x.lib().fewbit_hipx_glu_backward_product, torch.cuda.current_stream().cuda_stream
        act = cabi.CONTINUOUS.index(activation)
        rc = f(cabi.DTYPES[dtype], act, gyd.data_ptr(), state.data_ptr(), rows, width, bits, None, 0, D.t.data_ptr(), width, None, 0, stream)
        torch.cuda.synchronize()
        assert rc == 0 and D.intact() and same_bytes(D.t.view(rows, width), full[1])
        assert f(cabi.DTYPES[dtype], act, gyd.data_ptr(), state.data_ptr(), rows, width, bits, None, 0, None, 0, None, 0, stream) == 0
        assert cabi_x.glu_backward_product(gyd, state, activation, bits, (False, False, False)) == (None, None, None)


# ---- poisoned groups -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('activation', ACTIVATIONS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_non_finite_inputs_poison_whole_groups_of_all_three_outputs(dtype, activation):
    for bits in BITS:
        poisoned_groups_of_all_three_outputs(dtype, activation, bits)


def poisoned_groups_of_all_three_outputs(dtype, activation, bits):
    rows, width = 4, 80
    n = rows * width
    gate, up, gy = inputs(rows, width, dtype, 7)
    flat_g, flat_u = gate.view(-1), up.view(-1)
    flat_g[3], flat_g[70], flat_g[71], flat_u[130], flat_u[131], flat_u[319] = float('nan'), float('inf'), float('-inf'), float('inf'), float('nan'), float('-inf')
    _, state = cabi_x.glu_forward(gate.to(DEV), up.to(DEV), activation, bits, SEED)
    outs = cabi_x.glu_backward_product(gy.to(DEV), state, activation, bits)
    group = torch.arange(n) // 64
    poisoned = ((group == 0) | (group == 1) | (group == 2) | (group == 4)).view(rows, width)
    assert all(torch.equal(torch.isnan(t.cpu()), poisoned) for t in outs)
    # the other groups: to the bit what they are when the non-finite elements are ordinary numbers
    tame_g, tame_u = torch.nan_to_num(gate, 0.5, 0.5, 0.5), torch.nan_to_num(up, 0.5, 0.5, 0.5)
    _, tame_state = cabi_x.glu_forward(tame_g.to(DEV), tame_u.to(DEV), activation, bits, SEED)
    tame_outs = cabi_x.glu_backward_product(gy.to(DEV), tame_state, activation, bits)
    assert all(same_bytes(a.cpu()[~poisoned], b.cpu()[~poisoned]) for a, b in zip(outs, tame_outs))
    # the product alone, without gy
    P = torch.empty(rows, width, dtype=dtype, device=DEV)
    cabi_x.glu_backward_product(None, state, activation, bits, (False, False, True), product=P)
    assert torch.equal(torch.isnan(P.cpu()), poisoned) and same_bytes(P.cpu()[~poisoned], outs[2].cpu()[~poisoned])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', (torch.bfloat16, torch.float32))
def test_refusals_leave_the_buffers_untouched(dtype):
    rows, width, bits = 3, 24, 4
    gate, up, gy = (t.to(DEV) for t in inputs(rows, width, dtype))
    _, state = cabi_x.glu_forward(gate, up, 'silu', bits, SEED)
    D, U, P = (Guarded(rows * width, dtype) for _ in range(3))
    views = [b.t.view(rows, width) for b in (D, U, P)]
    with pytest.raises(cabi_x.FewbitHipError, match='at least'):
        cabi_x.glu_backward_product(gy, state[:-8], 'silu', bits, (True, True, True), *views)
    with pytest.raises(cabi_x.FewbitHipError, match='bits must be 2, 4 or 8'):
        cabi_x.glu_backward_product(gy, state, 'silu', 3, (True, True, True), *views)
    with pytest.raises(cabi_x.FewbitHipError, match="'silu' or 'gelu'"):
        cabi_x.glu_backward_product(gy, state, 'gelu_tanh', bits, (True, True, True), *views)
    with pytest.raises(cabi_x.FewbitHipError, match='neither d_gate nor d_up'):
        cabi_x.glu_backward_product(None, state, 'silu', bits, (False, True, True), *views)
    with pytest.raises(cabi_x.FewbitHipError, match='must be a 3 x 24 tensor'):
        cabi_x.glu_backward_product(gy, state, 'silu', bits, (True, True, True), views[0], views[1], P.t.view(width, rows))
    with pytest.raises(cabi_x.FewbitHipError, match='unit stride'):
        cabi_x.glu_backward_product(gy, state, 'silu', bits, (False, False, True), product=torch.empty(width, rows, dtype=dtype, device=DEV).t())
    f, stream = cabi_x.lib().fewbit_hipx_glu_backward_product, torch.cuda.current_stream().cuda_stream
    ok = dict(dtype=cabi.DTYPES[dtype], act=cabi.CONTINUOUS.index('silu'), gy=gy.data_ptr(), state=state.data_ptr(), rows=rows, width=width, bits=bits, d_gate=D.t.data_ptr(), ld_dgate=width,
              d_up=U.t.data_ptr(), ld_dup=width, product=P.t.data_ptr(), ld_product=width, stream=stream)
    for changed in (dict(bits=5), dict(ld_product=8), dict(dtype=5), dict(act=0), dict(gy=None), dict(gy=None, d_gate=None),
                    dict(product=P.t.data_ptr() + P.t.element_size() // 2)):          # (half an element off: 1 byte for bf16, 2 for fp32)
        assert f(*{**ok, **changed}.values()) == -1, changed
    torch.cuda.synchronize()
    assert D.unchanged() and U.unchanged() and P.unchanged()
