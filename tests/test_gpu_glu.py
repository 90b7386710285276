"""The kernels of the gated product on the GPU (fewbit_amd/csrc/fewbit_glu.hip) against the host evaluation and float64: the state bit for bit
``glu_state_host`` at the sizes where the plan changes, ``y`` and both gradients within the bounds of the definition, guard bytes around every
output, untouched row gaps, non-finite inputs, absent outputs, refusals, and a captured forward + backward.

The bounds.  16-bit ``y`` and ``d_up``: ``|got - R| <= (h + 2^-20) |R| + the smallest subnormal`` with ``h`` half an ulp (2^-8 for bf16, 2^-11 for
fp16) and 2^-20 the fp32 error allowed to the evaluation of ``act``.  fp32 ``y`` and ``d_up``: the largest error in ulps is at most that of torch's
own fp32 ``act(g) * u`` on the same tensors plus 2.  ``d_gate = (gy u^) act'(g^)``: the formula of ``act'`` ADDS terms of both signs (it is 0 near
g = -1.28 for silu and near g = -0.75 for gelu), so its fp32 error is relative to the sum of the magnitudes of those terms, not to their sum: the
2^-20 is taken of ``|gy u^| * (the magnitudes, glu_harness.slope_terms64)``, the half ulp of the dtype stays relative to ``R``.

MEASURED on an MI355X (see EXPERIMENTS.md section 8.22): the figures each test prints."""
import math

import pytest
import torch

from fewbit_amd import cabi, cabi_x
from glu_harness import FAST_CLASS, TINY, UNIT, act64, decoded, slope64, slope_terms64, torch_act, ulp_error
from norm_harness import DEV, Guarded

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.float16, torch.bfloat16)
BITS = (2, 4, 8)
ACTIVATIONS = ('silu', 'gelu')
SEED = 0x0123456789abcdef


class Strided:
    """a logical rows x width matrix whose rows are `ld` elements apart, `off` elements behind a 256-byte aligned address, in a guarded buffer that
    ends with the last element of the last row; every byte of it is the sentinel until `values` are written"""

    def __init__(self, rows, width, ld, dtype, off=0, values=None):
        self.buffer = Guarded((rows - 1) * ld + width, dtype, off)
        self.view = self.buffer.t.as_strided((rows, width), (ld, 1))
        if values is not None:
            self.view.copy_(values)
            self.buffer.before = self.buffer.raw.clone()

    def only_the_matrix_was_written(self):
        """the guards, and the gaps between the rows, hold what they held"""
        after = self.buffer.raw.clone()
        was = self.buffer.before[self.buffer.lo:self.buffer.hi].view(self.view.dtype).as_strided(self.view.shape, self.view.stride())
        after[self.buffer.lo:self.buffer.hi].view(self.view.dtype).as_strided(self.view.shape, self.view.stride()).copy_(was)
        return torch.equal(after, self.buffer.before)


def inputs(rows, width, dtype, salt=0):
    g = torch.Generator().manual_seed(1000 * rows + width + salt)
    return tuple((3 * torch.randn(rows, width, generator=g)).to(dtype) for _ in range(3))


def within_16_bit_bound(got, exact, dtype, fp32_error_of=None):
    fp32_error_of = exact.abs() if fp32_error_of is None else fp32_error_of
    return (got.double() - exact).abs() <= UNIT[dtype] * exact.abs() + FAST_CLASS * fp32_error_of + TINY[dtype]


def check_y(y, gate, up, activation, dtype, label):
    exact = act64(gate, activation) * up.double()
    if dtype == torch.float32:
        ours, torchs = ulp_error(y, exact), ulp_error(torch_act(gate.to(DEV), activation).cpu() * up, exact)
        print(f'{label} y: max error {float(ours.max()):.2f} ulp, torch {float(torchs.max()):.2f} ulp')
        assert float(ours.max()) <= float(torchs.max()) + 2.0, label
    else:
        excess = ((y.double() - exact).abs() - TINY[dtype]) / exact.abs().clamp_min(1e-300)
        print(f'{label} y: max relative error {float(excess.max()) / UNIT[dtype]:.4f} half ulps (bound 1 + {FAST_CLASS / UNIT[dtype]:.4f})')
        assert bool(within_16_bit_bound(y, exact, dtype).all()), label


def check_gradients(d_gate, d_up, gy, gq, uq, activation, dtype, label):
    """against the float64 formula on the host decode (module docstring)"""
    want_up = gy.double() * act64(gq, activation)
    pair = gy.double() * uq.double()
    want_gate, terms = pair * slope64(gq, activation), pair.abs() * slope_terms64(gq, activation)
    if dtype == torch.float32:
        ours, torchs = ulp_error(d_up, want_up), ulp_error(gy * torch_act(gq.to(DEV), activation).cpu(), want_up)
        print(f'{label} d_up: max error {float(ours.max()):.2f} ulp, torch {float(torchs.max()):.2f} ulp')
        assert float(ours.max()) <= float(torchs.max()) + 2.0, label
        worst = ((d_gate.double() - want_gate).abs() - UNIT[dtype] * want_gate.abs()) / terms.clamp_min(1e-300)
        print(f'{label} d_gate: max error beyond half an ulp {float(worst.max()) / 2.0**-24:.2f} fp32 ulps of the terms')
    else:
        assert bool(within_16_bit_bound(d_up, want_up, dtype).all()), label + ' d_up'
    assert bool(within_16_bit_bound(d_gate, want_gate, dtype, terms).all()), label + ' d_gate'


def run(rows, width, ld_gate, ld_up, off, dtype, bits, activation, device_word=False, salt=0, check_values=False):
    """one forward (with a state and plain) and one backward in guarded, strided buffers: the state against the host evaluation, the guards, the gaps;
    with `check_values`, y and both gradients against float64"""
    label = f'{rows}x{width} ld {ld_gate}/{ld_up} off {off} {dtype} bits {bits} {activation}'
    n = rows * width
    gate, up, gy = inputs(rows, width, dtype, salt)
    G, U = Strided(rows, width, ld_gate, dtype, off, gate.to(DEV)), Strided(rows, width, ld_up, dtype, off, up.to(DEV))
    Y, S = Guarded(n, dtype, off), Guarded(cabi_x.glu_state_bytes(n, bits), torch.uint8)
    seed = torch.tensor([SEED], dtype=torch.int64, device=DEV) if device_word else SEED
    y, state = cabi_x.glu_forward(G.view, U.view, activation, bits, seed, y=Y.t.view(rows, width), state=S.t)
    torch.cuda.synchronize()
    assert Y.intact() and S.intact() and G.buffer.unchanged() and U.buffer.unchanged(), label
    host = cabi_x.glu_state_host(gate.float(), up.float(), SEED, bits)
    assert torch.equal(state.cpu(), host), (label, torch.nonzero(state.cpu() != host)[:8].flatten().tolist())
    # the plain forward: the same bytes of y, no state
    Y2 = Guarded(n, dtype, off)
    y2, none = cabi_x.glu_forward(G.view, U.view, activation, keep=False, y=Y2.t.view(rows, width))
    assert none is None and torch.equal(y2.view(torch.uint8), y.view(torch.uint8)) and Y2.intact(), label
    # backward into strided outputs: the gaps and the guards keep their sentinels
    GY = Guarded(n, dtype, off, like=gy.to(DEV))
    DG, DU = Strided(rows, width, ld_gate, dtype, off), Strided(rows, width, ld_up, dtype, off)
    d_gate, d_up = cabi_x.glu_backward(GY.t.view(rows, width), state, activation, bits, d_gate=DG.view, d_up=DU.view)
    torch.cuda.synchronize()
    assert DG.only_the_matrix_was_written() and DU.only_the_matrix_was_written() and GY.unchanged() and S.intact(), label
    if check_values:
        check_y(y.cpu(), gate, up, activation, dtype, label)
        gq, uq = decoded(host, n, bits)
        check_gradients(d_gate.cpu(), d_up.cpu(), gy, gq.view(rows, width), uq.view(rows, width), activation, dtype, label)
    return y, state, d_gate.clone(), d_up.clone()


def combinations():
    return [(dtype, bits, activation) for dtype in DTYPES for bits in BITS for activation in ACTIVATIONS]


# ---- the state, y and the gradients at every size at which the kernels take another path ------------------------------------------------------------
@pytest.mark.parametrize('n', (1, 7, 8, 9, 63, 64, 65))
def test_one_row(n):
    for i, (dtype, bits, activation) in enumerate(combinations()):
        run(1, n, n, n, 0, dtype, bits, activation, device_word=bool(i & 1))


@pytest.mark.parametrize('rows,width', ((3, 24), (5, 72)))
def test_the_halves_of_a_matrix_of_144_columns(rows, width):
    """row stride 144, 16-byte aligned: the vector path steps over the gap"""
    for dtype, bits, activation in combinations():
        strided = run(rows, width, 144, 144, 0, dtype, bits, activation)
        dense = run(rows, width, width, width, 0, dtype, bits, activation)
        assert all(torch.equal(a, b) for a, b in zip(strided, dense))


def test_blocks_that_straddle_rows_take_the_element_path():
    for dtype, bits, activation in combinations():
        run(2, 100, 100, 100, 0, dtype, bits, activation)
        run(2, 100, 100, 104, 0, dtype, bits, activation, salt=1)


def test_a_base_one_element_off_takes_the_element_path_with_the_same_bytes():
    for dtype, bits, activation in combinations():
        y0, aligned, dg0, du0 = run(3, 24, 24, 24, 0, dtype, bits, activation)
        y1, state, dg1, du1 = run(3, 24, 24, 24, 1, dtype, bits, activation)
        assert torch.equal(y0, y1) and torch.equal(state, aligned) and torch.equal(dg0, dg1) and torch.equal(du0, du1)
        y2, state, dg2, du2 = run(3, 24, 40, 32, 1, dtype, bits, activation)
        assert torch.equal(y0, y2) and torch.equal(state, aligned) and torch.equal(dg0, dg2) and torch.equal(du0, du2)


def test_a_lane_takes_a_second_sweep():
    n = cabi_x.QUANT_SWEEP + 8 + 3
    for dtype, bits, activation in zip(DTYPES, BITS, ('silu', 'gelu', 'silu')):
        run(1, n, n, n, 0, dtype, bits, activation)


@pytest.mark.parametrize('activation', ACTIVATIONS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_y_and_the_gradients_against_float64(dtype, activation):
    """3 N(0, 1) inputs on the vector path (16 x 256) and on the element path (2 x 100 with a gap behind the rows of up, one row of 65): the figures of
    EXPERIMENTS.md section 8.22.

    MEASURED on an MI355X at 16 x 256.  silu: y within 0.994 of the bound's half ulp for bf16 and fp16 (the bound: 1.0002 and 1.002 half ulps); fp32 y at
    most 2.06 ulp, torch's own 2.06; fp32 d_up 2.46 ulp, torch's 2.46; d_gate at most 9.5 fp32 ulps of its terms (allowed: 16).  gelu, fp32: the maxima
    are torch's to the digit (1.67e7 ulp for both: g * 0.5 * (1 + erf(g / sqrt 2)) is 0 where erf rounds to -1, at g < -5.6, in torch as here).
    gelu with bf16 and fp16 I/O: y within 0.999 of the bound's half ulp (its negative tail is an erfc with a compensated argument; the fast class's
    gelu_fast, accurate to 2^-21 |g|, gave 256 half ulps for bf16 and 18.4 for fp16 here).  These inputs hold no gate beyond about +-13: EVERY bf16 and
    fp16 gate, against 21 ups, is tests/test_gpu_glu_values.py (EXPERIMENTS.md section 8.24), for silu as for gelu."""
    for bits in BITS:
        run(16, 256, 256, 256, 0, dtype, bits, activation, salt=bits, check_values=True)
        run(2, 100, 100, 104, 0, dtype, bits, activation, salt=bits, check_values=True)
        run(1, 65, 65, 65, 0, dtype, bits, activation, salt=bits, check_values=True)


# ---- non-finite values, absent outputs, refusals -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('activation', ACTIVATIONS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_non_finite_inputs_poison_whole_groups_of_the_gradients_only(dtype, activation):
    rows, width, bits = 4, 80, 4
    n = rows * width
    gate, up, gy = inputs(rows, width, dtype, 7)
    flat_g, flat_u = gate.view(-1), up.view(-1)
    flat_g[3], flat_g[70], flat_g[71], flat_u[130], flat_u[131], flat_u[319] = float('nan'), float('inf'), float('-inf'), float('inf'), float('nan'), float('-inf')
    flat_g[200:204], flat_u[202:206] = torch.tensor([0.0, -0.0, 0.0, -0.0]), torch.tensor([-0.0, 0.0, 1.0, -0.0])
    flat_u[70], flat_u[71] = 0.0, 2.0
    y, state = cabi_x.glu_forward(gate.to(DEV), up.to(DEV), activation, bits, SEED)
    assert torch.equal(state.cpu(), cabi_x.glu_state_host(gate.float(), up.float(), SEED, bits))
    exact = act64(gate, activation) * up.double()
    assert torch.equal(torch.isnan(y.cpu()), torch.isnan(exact))                       # y: the exact forward, NaN where float64 has one
    assert bool((y.cpu().view(-1)[200:204] == 0).all())                                # +-0 * finite
    d_gate, d_up = cabi_x.glu_backward(gy.to(DEV), state, activation, bits)
    group = torch.arange(n) // 64
    poisoned = ((group == 0) | (group == 1) | (group == 2) | (group == 4)).view(rows, width)
    assert torch.equal(torch.isnan(d_gate.cpu()), poisoned) and torch.equal(torch.isnan(d_up.cpu()), poisoned)
    # the other groups: to the bit what they are when the non-finite elements are ordinary numbers
    tame_g, tame_u = torch.nan_to_num(gate, 0.5, 0.5, 0.5), torch.nan_to_num(up, 0.5, 0.5, 0.5)
    _, tame_state = cabi_x.glu_forward(tame_g.to(DEV), tame_u.to(DEV), activation, bits, SEED)
    tame_gate, tame_up = cabi_x.glu_backward(gy.to(DEV), tame_state, activation, bits)
    assert torch.equal(d_gate.cpu()[~poisoned], tame_gate.cpu()[~poisoned]) and torch.equal(d_up.cpu()[~poisoned], tame_up.cpu()[~poisoned])


def test_an_absent_gradient_is_skipped_and_left_untouched():
    rows, width, bits = 5, 72, 4
    for dtype, activation in zip(DTYPES, ('silu', 'gelu', 'silu')):
        gate, up, gy = inputs(rows, width, dtype, 3)
        _, state = cabi_x.glu_forward(gate.to(DEV), up.to(DEV), activation, bits, SEED)
        both = cabi_x.glu_backward(gy.to(DEV), state, activation, bits)
        for want in ((True, False), (False, True)):
            outs = cabi_x.glu_backward(gy.to(DEV), state, activation, bits, want)
            for got, full, wanted in zip(outs, both, want):
                assert (got is None) != wanted and (got is None or torch.equal(got, full))
        # through the entry point itself: a NULL output next to a guarded one
        D = Guarded(rows * width, dtype)
        gyd = gy.to(DEV)
        rc = cabi_x.lib().fewbit_hipx_glu_backward(cabi.DTYPES[dtype], cabi.CONTINUOUS.index(activation), gyd.data_ptr(), state.data_ptr(), rows, width, bits, None, 0,
                                                   D.t.data_ptr(), width, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0 and D.intact() and torch.equal(D.t.view(rows, width), both[1])
        assert cabi_x.glu_backward(gy.to(DEV), state, activation, bits, (False, False)) == (None, None)


def test_refusals_leave_the_buffers_untouched():
    rows, width, bits, dtype = 3, 24, 4, torch.bfloat16
    gate, up, gy = (t.to(DEV) for t in inputs(rows, width, dtype))
    Y, S = Guarded(rows * width, dtype), Guarded(cabi_x.glu_state_bytes(rows * width, bits) - 8, torch.uint8)
    with pytest.raises(cabi_x.FewbitHipError, match='are needed'):
        cabi_x.glu_forward(gate, up, 'silu', bits, SEED, y=Y.t.view(rows, width), state=S.t)
    with pytest.raises(cabi_x.FewbitHipError, match='bits must be 2, 4 or 8'):
        cabi_x.glu_forward(gate, up, 'silu', 3, SEED, y=Y.t.view(rows, width))
    with pytest.raises(cabi_x.FewbitHipError, match="'silu' or 'gelu'"):
        cabi_x.glu_forward(gate, up, 'gelu_tanh', bits, SEED, y=Y.t.view(rows, width))
    with pytest.raises(cabi_x.FewbitHipError, match='shape and dtype of gate'):
        cabi_x.glu_forward(gate, up.float(), 'silu', bits, SEED, y=Y.t.view(rows, width))
    with pytest.raises(cabi_x.FewbitHipError, match='unit stride'):
        cabi_x.glu_forward(gate.t().contiguous().t(), up, 'silu', bits, SEED, y=Y.t.view(rows, width))
    L, stream = cabi_x.lib(), torch.cuda.current_stream().cuda_stream
    for changed in (dict(bits=3), dict(ld=8), dict(dt=5), dict(act=0)):
        rc = L.fewbit_hipx_glu_forward(changed.get('dt', 2), changed.get('act', 8), gate.data_ptr(), changed.get('ld', width), up.data_ptr(), width, rows, width,
                                       changed.get('bits', bits), SEED, None, Y.t.data_ptr(), S.t.data_ptr(), 10**6, stream)
        assert rc == -1, changed
    D = Guarded(rows * width, dtype)
    state = torch.zeros(cabi_x.glu_state_bytes(rows * width, bits), dtype=torch.uint8, device=DEV)
    with pytest.raises(cabi_x.FewbitHipError, match='at least'):
        cabi_x.glu_backward(gy, state[:-8], 'silu', bits, d_up=D.t.view(rows, width))
    assert L.fewbit_hipx_glu_backward(2, 8, gy.data_ptr(), state.data_ptr(), rows, width, 5, D.t.data_ptr(), width, D.t.data_ptr(), width, stream) == -1
    torch.cuda.synchronize()
    assert Y.unchanged() and S.unchanged() and D.unchanged()
    empty = torch.empty(0, width, dtype=dtype, device=DEV)
    y, state = cabi_x.glu_forward(empty, empty, 'silu', bits, SEED)
    assert y.shape == (0, width) and state.numel() == 0


# ---- a captured forward + backward --------------------------------------------------------------------------------------------------------------------
def test_a_captured_forward_and_backward_round_afresh_on_every_replay():
    rows, width, bits, dtype, base = 5, 72, 4, torch.bfloat16, 0x2468ace
    gate, up, gy = inputs(rows, width, dtype, 9)
    gd, ud, gyd = gate.to(DEV), up.to(DEV), gy.to(DEV)
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)

    def step():
        word = cabi.next_sketch_seed(counter, base)
        y, state = cabi_x.glu_forward(gd, ud, 'silu', bits, word)
        return (y, state) + cabi_x.glu_backward(gyd, state, 'silu', bits)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    c0 = int(counter)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, state, d_gate, d_up = step()
    states = []
    for replay in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert int(counter) == c0 + replay + 1
        seed = cabi.mix_sketch_seed(base, c0 + replay)
        assert torch.equal(state.cpu(), cabi_x.glu_state_host(gate.float(), up.float(), seed, bits))
        ye, se = cabi_x.glu_forward(gd, ud, 'silu', bits, seed)
        dge, due = cabi_x.glu_backward(gyd, se, 'silu', bits)
        assert torch.equal(y, ye) and torch.equal(d_gate, dge) and torch.equal(d_up, due)
        states.append(state.clone())
    assert not torch.equal(states[0], states[1])
    assert math.isfinite(float(d_gate.float().abs().sum()))
