"""What the tests of the two quantized norms share (tests/test_gpu_norm.py, test_gpu_norm_layer.py, test_norm_host.py and their ``rms_`` twins;
``philox`` and ``order_keys`` also serve tests/test_quant_host.py): guarded GPU buffers and the options of a sweep, the hooks that show what a
call saved and which seeds it drew, the numpy pieces of the definition, the two statistics over many calls, and -- as functions of a ``Kind``, the
record of what differs between the layer norm and the RMS norm -- the bodies that are one text for both: the layer inside checkpointing,
autocast, no_grad / eval and a captured graph, and the gradients of 200 calls on host tensors; the row counts at which a workgroup of the entry
points walks on to a later tile (``walk``), the tables of such cases and the two bodies that run them through a module's own ``run_*`` and
``check_*``.  Wherever the two kinds assert different things (bounds, non-finite patterns) the tests stay in their own files."""
import math
from typing import Callable, NamedTuple

import numpy as np
import pytest
import torch
from torch.utils.checkpoint import checkpoint

import fewbit
from fewbit_amd import cabi, cabi_x, linear

DEV = 'cuda:0'
UNIT = {torch.float32: 2.0**-24, torch.float16: 2.0**-11, torch.bfloat16: 2.0**-8}
EPS = 1e-5
SEED = 0x0123456789abcdef
FILL = 0xA5
M32 = np.uint64(0xffffffff)


class Kind(NamedTuple):
    """one of the two norms.  The parameters of a call are a tuple, ``(weight, bias)`` or ``(weight, )``, that is spliced in behind the input of
    ``functional`` (..., eps, bits, generator) and of ``forward`` (..., eps, bits, seed)"""
    functional: Callable          # fewbit.functional.*_norm_quantized(x, normalized_shape, *parameters, eps, bits, generator)
    module: type                  # fewbit.Quantized*Norm
    forward: Callable             # cabi_x.*_norm_forward(x, *parameters, eps, bits, seed) -> (y, rstd, state, xhat)
    backward: Callable            # cabi_x.*_norm_backward(gy, state, rstd, gamma, bits) -> (dx, dgamma[, dbeta])
    node: str                     # the name of the grad_fn
    centred: bool

    def exact_rows(self, x, eps):
        """(x^, rstd) in float64"""
        x = x.double()
        if self.centred:
            x = x - x.mean(dim=1, keepdim=True)
        rstd = 1.0 / torch.sqrt(x.square().mean(dim=1, keepdim=True) + eps)
        return x * rstd, rstd.reshape(-1)

    def formula64(self, gy, xq, rstd, gamma):
        """(dx, dgamma[, dbeta]) of the definition in float64"""
        gy, xq, rstd = gy.double(), xq.double(), rstd.double()
        gh = gy * gamma.double() if gamma is not None else gy
        if not self.centred:
            return rstd[:, None] * (gh - xq * (gh * xq).mean(dim=1, keepdim=True)), (gy * xq).sum(dim=0)
        dx = rstd[:, None] * (gh - gh.mean(dim=1, keepdim=True) - xq * (gh * xq).mean(dim=1, keepdim=True))
        return dx, (gy * xq).sum(dim=0), gy.sum(dim=0)


LAYER_NORM = Kind(fewbit.functional.layer_norm_quantized, fewbit.QuantizedLayerNorm, cabi_x.layer_norm_forward, cabi_x.layer_norm_backward,
                  '_LayerNormQuantizedBackward', True)
RMS_NORM = Kind(fewbit.functional.rms_norm_quantized, fewbit.QuantizedRMSNorm, cabi_x.rms_norm_forward, cabi_x.rms_norm_backward,
                '_RMSNormQuantizedBackward', False)


# ---- guarded buffers and the options of a sweep of the entry points ---------------------------------------------------------------------------
class Guarded:
    """`numel` elements of `dtype` on the GPU, `off` elements behind a 256-byte aligned address, between 256 guard bytes on either side"""

    def __init__(self, numel, dtype, off=0, like=None):
        item = torch.empty(0, dtype=dtype).element_size()
        self.lo = 256 + off * item
        self.hi = self.lo + numel * item
        self.raw = torch.full((self.hi + 256, ), FILL, dtype=torch.uint8, device=DEV)
        assert self.raw.data_ptr() % 256 == 0
        self.t = self.raw[self.lo:self.hi].view(dtype)
        if like is not None:
            self.t.copy_(like.reshape(-1))
        self.before = self.raw.clone()

    def intact(self):
        return bool((self.raw[:self.lo] == FILL).all()) and bool((self.raw[self.hi:] == FILL).all())

    def unchanged(self):
        return torch.equal(self.raw, self.before)


def options(i):
    """offset from 16-byte alignment (elements), the affine parameters present, the seed as a device word: every combination within 8 cases"""
    return i & 1, bool((i >> 1) & 1), bool((i >> 2) & 1)


def seed_argument(device_word):
    return torch.tensor([SEED], dtype=torch.int64, device=DEV) if device_word else SEED


def allowance(measured, width):
    return max(2.0 * measured, math.log2(width) + 4.0)


# ---- where a workgroup begins to walk ------------------------------------------------------------------------------------------------------------
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
BITS = (2, 4, 8)
CAP = {'forward': 16384, 'backward': 512}       # kMaxGridForward, kMaxGridBackward of fewbit_norm.hip: the most workgroups a launch has
LANES = {'forward': 256, 'backward': 1024}      # kThreads, kBackwardThreads: the lanes of a workgroup


def lanes_per_row(width, direction):
    """``cabi_x.norm_plan``'s lanes forward; backward a lane holds ONE block, so beyond 2048 elements a row takes 512 or 1024 lanes (its docstring)"""
    lanes, blocks = cabi_x.norm_plan(width)
    return lanes if direction == 'forward' else lanes * blocks


def walk(width, direction, tiles, extra=None):
    """The rows at which a workgroup of `direction` ('forward' / 'backward') at `width` takes its tile number `tiles`:
    ``(tiles - 1) * cap * rows_per_tile + extra`` with rows_per_tile = 256 / lanes forward and 1024 / lanes backward (lanes: ``norm_plan``'s, and the
    backward rule of its docstring) and cap = 16384 workgroups forward, 512 backward -- the constants of fewbit_norm.hip that ``norm_plan`` quotes.
    `extra` rows go into the last sweep: 1 makes workgroup 0 alone walk on, with one live row in its tile; None is a full sweep, every workgroup
    walks.  Backward the walk is asserted from the library: the workspace is that of a grid at its cap, and there are more tiles than that."""
    lanes = lanes_per_row(width, direction)
    per_tile, cap = LANES[direction] // lanes, CAP[direction]
    extra = cap * per_tile if extra is None else extra
    assert tiles >= 2 and 1 <= extra <= cap * per_tile
    rows = (tiles - 1) * cap * per_tile + extra
    if direction == 'backward':
        assert cabi_x.norm_workspace_bytes(rows, width) == 512 * 2 * lanes * 8 * 4, f'{rows} x {width}: the backward grid is not 512 workgroups of {lanes} lanes per row'
        assert -(-rows // per_tile) > 512, f'{rows} x {width}: no workgroup takes a second tile'
    return rows


class Walk(NamedTuple):
    lanes: int                    # per row
    blocks: int                   # of 8 elements per lane
    width: int
    tiles: int                    # the tile of its walk that workgroup 0 reaches
    extra: object                 # rows in the last sweep; None: a full one
    dtype: torch.dtype
    bits: int
    off: int                      # elements off 16-byte alignment
    affine: bool

    def rows(self, direction):
        rows = walk(self.width, direction, self.tiles, self.extra)
        assert (self.lanes, self.blocks) == (lanes_per_row(self.width, direction), 1 if direction == 'backward' else cabi_x.norm_plan(self.width)[1])
        return rows

    def __str__(self):
        return f'{self.lanes}x{self.blocks}-w{self.width}-{self.tiles}_tiles{"" if self.extra is None else "+%d" % self.extra}-{str(self.dtype)[6:]}-{self.bits}b'


# backward: (lanes per row, widths, (tile reached, rows of the last sweep)); every width with every row count.  Width 4097 runs one element off
# 16-byte alignment (its rows are off it by themselves from the second on)
BACKWARD_WALKS = ((16, (72, 128), ((2, 1), (3, 1))), (64, (136, 192), ((2, 1), (3, 1))), (256, (1032, 2048), ((2, 1), (3, 1), (3, None))),
                  (512, (2056, 4096), ((2, 1), (3, 1), (3, None))), (1024, (4104, 8192, 4097), ((2, 1), (3, 1), (3, None))))
# forward: ((lanes per row, blocks per lane), widths, (tile reached, rows of the last sweep)); 136 and 1032 keep a short last group inside a walk
FORWARD_WALKS = (((16, 1), (128, ), ((2, 1), )), ((64, 1), (192, 136), ((2, 1), )), ((256, 1), (1088, 1032), ((2, 1), (3, 1))),
                 ((256, 2), (2112, ), ((2, 1), )), ((256, 4), (4160, ), ((2, 1), )))


def walks(direction, shift=0, fused=False):
    """The cases of a table.  dtype and bits rotate over the cases of a plan (`shift`: where the rotation starts, so that the two kinds differ) such
    that the plain cases of ONE kind hold every (plan, dtype) and every (plan, bits) pair: a plan with fewer than three cases repeats them with the
    next dtype and bits.  The forward plan of four blocks per lane runs in the 16-bit dtypes, which halves its input.  `fused`: ONE width per
    plan -- `shift` picks which -- with every row count once, and forward only the plans of 256 lanes per row (1, 2 and 4 blocks per lane)."""
    for plan, widths, sweeps in FORWARD_WALKS if direction == 'forward' else BACKWARD_WALKS:
        lanes, blocks = plan if direction == 'forward' else (plan, 1)
        if fused and direction == 'forward' and lanes < 256:
            continue
        base = [(w, t, e) for w in ((widths[shift % len(widths)], ) if fused else widths) for t, e in sweeps]
        dtypes = DTYPES[1:] if blocks == 4 else DTYPES
        for i in range(len(base) if fused else max(3, len(base))):
            width, tiles, extra = base[i % len(base)]
            j = i + shift
            yield Walk(lanes, blocks, width, tiles, extra, dtypes[j % len(dtypes)], BITS[(j + i // 3) % 3], 1 if width % 4 else i & 1, i % 4 != 3)


def first_difference(a, b, row_bytes=None):
    """where two tensors of the same bytes first differ, for the message of a failed byte comparison ('' when equal): flat byte offsets, and the
    rows they lie in when a row has `row_bytes` bytes"""
    a, b = a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8)
    if a.numel() != b.numel():
        return f'{a.numel()} against {b.numel()} bytes'
    at = torch.nonzero(a != b).flatten()
    if at.numel() == 0:
        return ''
    rows = '' if row_bytes is None else f', rows {sorted(set((at[:64] // row_bytes).tolist()))[:8]}'
    return f'{at.numel()} bytes differ, the first at {at[:8].tolist()}{rows}'


def state_rows(state, rows, width):
    """the bytes of a state row by row: (the (lo, step) pairs, the codes)"""
    pairs = 8 * rows * -(-width // 64)
    return state[:pairs].view(rows, -1), state[pairs:].view(rows, -1)


def backward_walks_on(case, backward_problem, run_backward, check_backward_values):
    """A backward workgroup on a later tile of its walk, from the host state of a module's `backward_problem` through its `run_backward` (guards
    intact, inputs unchanged) and `check_backward_values` (the float64 formula, the unchanged bounds); two runs byte-equal -> (K', the torch ops')"""
    rows, width = case.rows('backward'), case.width
    state, xq, rstd, gy, gamma = backward_problem(rows, width, case.dtype, case.bits, case.affine)
    outs = run_backward(state, rstd, gy, gamma, case.bits, case.off)
    k = check_backward_values(xq, rstd, gy, gamma, outs[0].t.view(rows, width), *(o.t for o in outs[1:]), f'{rows} x {width} ({case})')
    again = run_backward(state, rstd, gy, gamma, case.bits, case.off)
    for name, a, b in zip(('dx', 'dgamma', 'dbeta'), outs, again):
        assert torch.equal(a.raw, b.raw), f'{rows} x {width} ({case}): two runs differ in {name}: {first_difference(a.t, b.t, width * a.t.element_size() if name == "dx" else None)}'
    print(f"{rows} x {width} ({case}): K'(dx) = {k[0]:.2f}; plain fp32 torch ops: {k[1]:.2f}")
    return k


def tiled(small, rows):
    """`rows` rows on the GPU: row r is row r % len(small) of `small`, and the index that says so"""
    index = torch.arange(rows, device=DEV) % small.shape[0]
    return small.to(DEV)[index], index


def forward_walks_on(case, inputs, run_forward, check_forward_values):
    """A forward workgroup on a later tile of its walk.  The input is the 37 distinct rows of a module's `inputs` repeated.  The 37 rows alone, a call
    of their own, are held to float64 by the module's `check_forward_values`; the plan is a function of the width alone and a row's arithmetic does not
    depend on its tile, so row r of the long call has the BYTES of row r % 37 of the short one in y, rstd and x^.  The state depends on r through
    the Philox counter: for a width that is a multiple of 64 it is ``quant_pack`` of the flat x^ (the header; tests/test_gpu_quant.py pins that to the
    host evaluation), for a ragged width ``norm_state_host`` in full.  Two runs byte-equal; ``keep=False`` gives the same y and rstd bytes."""
    rows, width = case.rows('forward'), case.width
    label = f'{rows} x {width} ({case})'
    small, *parameters = inputs(37, width, case.dtype)
    parameters = parameters if case.affine else [None] * len(parameters)
    y0, rstd0, _, xhat0 = run_forward(small, *parameters, case.bits, SEED, case.off)
    k = check_forward_values(small, *parameters, y0.t.view(37, width), rstd0.t, xhat0.t.view(37, width), f'37 x {width} ({case})')
    x, index = tiled(small, rows)
    y, rstd, state, xhat = run_forward(x, *parameters, case.bits, SEED, case.off)
    for name, long, short in (('y', y, y0), ('rstd', rstd, rstd0), ('xhat', xhat, xhat0)):
        a, b = long.t.view(rows, -1), short.t.view(37, -1)[index]
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f'{label}: {name} of row r is not that of row r % 37: {first_difference(a, b, a.shape[1] * a.element_size())}'
    if width % 64 == 0:
        want = cabi_x.quant_pack(xhat.t.clone(), SEED, case.bits)
    else:
        want = cabi_x.norm_state_host(xhat.t.view(rows, width).cpu(), SEED, case.bits).to(DEV)
    assert torch.equal(state.t, want), f'{label}: the state: {first_difference(state.t, want)}'
    plain = run_forward(x, *parameters, case.bits, SEED, case.off, keep=False, want_xhat=False)
    assert torch.equal(plain[0].raw, y.raw) and torch.equal(plain[1].raw, rstd.raw), f'{label}: keep=False: y {first_difference(plain[0].t, y.t)} rstd {first_difference(plain[1].t, rstd.t)}'
    again = run_forward(x, *parameters, case.bits, SEED, case.off)
    for name, a, b in zip(('y', 'rstd', 'state', 'xhat'), (y, rstd, state, xhat), again):
        assert torch.equal(a.raw, b.raw), f'{label}: two runs differ in {name}: {first_difference(a.t, b.t)}'
    print(f'37 x {width} ({case}): K(x^) = {k[0]:.2f}, K(rstd) = {k[1]:.2f}; plain fp32 torch ops: {k[2]:.2f}, {k[3]:.2f}')
    return k


# ---- what a call saved, which seeds it drew -----------------------------------------------------------------------------------------------------
def saved_by(call):
    """-> (result, the tensors autograd saved while `call` ran)"""
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        result = call()
    return result, saved


@pytest.fixture
def seeds(monkeypatch):
    """the seeds the layer draws, in order"""
    drawn = []
    real = linear._draw_seed

    def draw(generator):
        drawn.append(real(generator))
        return drawn[-1]

    monkeypatch.setattr(linear, '_draw_seed', draw)
    return drawn


# ---- the definition restated in numpy: the pieces every restatement needs ------------------------------------------------------------------------
def philox(c0, c1, c2, c3, seed):
    """Philox4x32-10 on arrays of counters (uint64 holding 32-bit words), key = the two halves of `seed`"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(seed & 0xffffffff), np.uint64((seed >> 32) & 0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def order_keys(x):
    """the order of the reals on float32 bits, -0 below +0"""
    b = x.view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7fffffff) - 1, b)


# ---- the statistics of the definition over many calls -----------------------------------------------------------------------------------------
CALLS = 200


def worst_standard_error(samples, exact):
    mean, sd = samples.mean(dim=0), samples.std(dim=0)
    assert bool((sd > 0).all())
    return float(((mean - exact).abs() / (sd / math.sqrt(samples.shape[0]))).max())


def ratio_of_the_mean(samples, exact):
    """R = |mean(dx_q) - dx| / (rms one-call error / sqrt(calls)): 1 for unbiased independent calls, sqrt(calls) for one reused seed"""
    one_call = math.sqrt(float((samples - exact).square().sum(dim=(1, 2)).mean()))
    return float((samples.mean(dim=0) - exact).norm()) / (one_call / math.sqrt(samples.shape[0])), one_call / float(exact.norm())


def gradients_over_calls(kind, rows, width, bits, salt=0):
    """-> (exact dx, exact dgamma, the dx and dgamma of CALLS calls, float64) for N(3, 2^2) inputs on the host, seeds from torch.manual_seed(0)"""
    g = torch.Generator().manual_seed(17 + salt)
    x = (3 + 2 * torch.randn(rows, width, generator=g)).requires_grad_()
    parameters = ((1 + 0.5 * torch.randn(width, generator=g)).requires_grad_(), )
    if kind.centred:
        parameters += (torch.randn(width, generator=g).requires_grad_(), )
    gy = torch.randn(rows, width, generator=g)
    xhat, rstd = kind.exact_rows(x.detach(), 1e-5)
    dx, dgamma = kind.formula64(gy, xhat, rstd, parameters[0].detach())[:2]
    torch.manual_seed(0)
    dxs, dgs = [], []
    for _ in range(CALLS):
        gx, gw = torch.autograd.grad(kind.functional(x, (width, ), *parameters, 1e-5, bits), (x, *parameters), gy)[:2]
        dxs.append(gx.double())
        dgs.append(gw.double())
    return dx, dgamma, torch.stack(dxs), torch.stack(dgs)


def weight_gradient_is_unbiased(kind, shape, bits):
    """Every entry of the mean dgamma of 200 calls within 5 standard errors of sum gy x^ (E[x^q] = x^, and dgamma is linear in x^q)"""
    _, dgamma, _, dgs = gradients_over_calls(kind, *shape, bits)
    z = worst_standard_error(dgs, dgamma)
    print(f'{shape} bits {bits}: worst entry of dgamma {z:.2f} standard errors')
    assert z <= 5.0


def input_gradient_averages_out(kind, shape, bits):
    """dx is NOT exactly unbiased: x^q enters it twice, E[dx_q] - dx = -rstd g^_i Var(x^q_i) / width, second order in the step.  R compares the
    deviation of the mean of 200 calls with the noise that mean would have if the calls were unbiased and independent (R = 1); a layer that
    reused one seed gives sqrt(200), about 14.  Bound: R <= 1.5, from width 64 on (the layer norm at (40, 8) and 2 bits: the bias itself gives 2.0)."""
    dx, _, dxs, _ = gradients_over_calls(kind, *shape, bits, 1)
    R, relative = ratio_of_the_mean(dxs, dx)
    print(f'{shape} bits {bits}: R = {R:.3f}, relative error of one call {relative:.5f}')
    assert R <= 1.5


# ---- the layer on the GPU inside training wrappers ----------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def native_sketch_on():
    """(autouse in the modules that import it by name)"""
    prev = linear.use_native_sketch(True)
    yield
    linear.use_native_sketch(prev)


def problem(kind, shape, dtype, salt=0):
    """-> (x, the parameters, gy) on the GPU; x and the parameters require grad"""
    g = torch.Generator().manual_seed(53 + salt)
    width = shape[-1]
    x = (3 + 2 * torch.randn(*shape, generator=g)).to(dtype).to(DEV).requires_grad_()
    parameters = ((1 + 0.5 * torch.randn(width, generator=g)).to(dtype).to(DEV).requires_grad_(), )
    if kind.centred:
        parameters += (torch.randn(width, generator=g).to(dtype).to(DEV).requires_grad_(), )
    gy = torch.randn(*shape, generator=g).to(dtype).to(DEV)
    return x, parameters, gy


def entry_points(kind, x, parameters, gy, bits, seed):
    """(y, (dx, dgamma[, dbeta]), state, rstd) of the entry points for `seed`"""
    flat = x.detach().reshape(-1, x.shape[-1]).contiguous()
    y, rstd, state, _ = kind.forward(flat, *(p.detach() for p in parameters), EPS, bits, seed)
    dx, *sums = kind.backward(gy.reshape(flat.shape).contiguous(), state, rstd, parameters[0].detach(), bits)
    return y.view(x.shape), (dx.view(x.shape), *sums), state, rstd


def checkpointing_gives_the_plain_runs_bits(kind, shape, reentrant):
    x, parameters, gy = problem(kind, shape, torch.bfloat16, 2)
    leaves = (x, *parameters)
    call = lambda t, *rest: kind.functional(t, (t.shape[-1], ), *rest, EPS, 4)
    torch.manual_seed(12)
    y0 = call(*leaves)
    plain = torch.autograd.grad(y0, leaves, gy)
    torch.manual_seed(12)
    y = checkpoint(call, *leaves, use_reentrant=reentrant)
    for leaf in leaves:
        leaf.grad = None
    y.backward(gy)
    assert torch.equal(y, y0)
    for leaf, want in zip(leaves, plain):
        assert torch.equal(leaf.grad, want)
    for leaf in leaves:
        leaf.grad = None


def backward_may_follow_the_autocast_block(kind, shape, seeds):
    """-> (x16, the fp32 parameters) for what a kind asserts on top"""
    x, parameters, gy = problem(kind, shape, torch.float32, 1)
    x16 = x.detach().bfloat16().requires_grad_()
    with torch.autocast('cuda', dtype=torch.bfloat16):
        y = kind.functional(x16, (x.shape[-1], ), *parameters, EPS, 4)
    assert y.dtype == torch.bfloat16 and type(y.grad_fn).__name__ == kind.node
    g16 = gy.bfloat16()
    gx, *sums = torch.autograd.grad(y, (x16, *parameters), g16)          # outside the block: the ordinary AMP pattern
    assert gx.dtype == torch.bfloat16 and all(s.dtype == torch.float32 for s in sums)
    ye, (dxe, *sums_e), _, _ = entry_points(kind, x16, tuple(p.bfloat16() for p in parameters), g16, 4, seeds[0])
    assert torch.equal(y, ye) and torch.equal(gx, dxe) and len(sums) == len(sums_e) and all(torch.equal(a, b) for a, b in zip(sums, sums_e))
    return x16, parameters


def no_grad_eval_and_frozen_parameters_build_no_node_and_keep_no_state(kind, x, seeds):
    layer = kind.module(x.shape[-1], eps=EPS, device=DEV, dtype=torch.bfloat16)
    y_train, _ = saved_by(lambda: layer(x))
    count = len(seeds)
    assert count == 1
    with torch.no_grad():
        y, saved = saved_by(lambda: layer(x))
    assert y.grad_fn is None and not saved and torch.equal(y, y_train)   # the plain forward: the same bytes
    layer.eval()
    y, saved = saved_by(lambda: layer(x))                                # eval: no state, no seed; gradients asked for there are torch's exact ones
    assert 'Quantized' not in type(y.grad_fn).__name__ and not any(t.dtype == torch.uint8 for t in saved) and len(seeds) == count
    with torch.no_grad():
        assert torch.equal(layer(x), y_train)
    layer.train()
    layer.requires_grad_(False)
    y, saved = saved_by(lambda: layer(x.detach()))
    assert y.grad_fn is None and not saved and torch.equal(y, y_train) and len(seeds) == count
    with torch.inference_mode():
        assert torch.equal(layer(x), y_train) and len(seeds) == count


def a_non_contiguous_input_is_normalized_from_a_contiguous_copy(kind, x, parameters, gy, seeds):
    base = torch.randn(x.shape[1], x.shape[0], device=DEV, dtype=torch.bfloat16)
    xt = base.t().requires_grad_()
    y = kind.functional(xt, (x.shape[-1], ), *parameters, EPS, 4)
    ye, (dxe, dge, *_), _, _ = entry_points(kind, xt, parameters, gy, 4, seeds[-1])
    gx, gw = torch.autograd.grad(y, (xt, parameters[0]), gy)
    assert torch.equal(y, ye) and torch.equal(gx, dxe) and torch.equal(gw, dge.bfloat16())


def a_captured_step_rounds_afresh_on_every_replay(kind, shape, monkeypatch):
    bits = 4
    x, parameters, gy = problem(kind, shape, torch.float32, 4)
    width = shape[-1]

    def step():
        y, saved = saved_by(lambda: kind.functional(x, (width, ), *parameters, EPS, bits))
        return (y, ) + torch.autograd.grad(y, (x, *parameters), gy) + (saved[0], saved[1])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                        # the eager warm-up: the per-device replay counter exists from here on
    torch.cuda.current_stream().wait_stream(side)
    bases = []
    monkeypatch.setattr(linear, '_draw_seed', lambda generator: bases.append(0x2468ace) or bases[-1])
    counter = linear._replay_counter(torch.device(DEV))
    torch.cuda.synchronize()
    c0 = int(counter)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y, *grads, state, rstd = step()
    assert len(bases) == 1 and int(counter) == c0
    seen = []
    for replay in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert int(counter) == c0 + replay + 1
        # each replay is consistent with its own state: the state of the seed the replay counter gave, and the gradients of that state
        ye, grads_e, state_e, rstd_e = entry_points(kind, x, parameters, gy, bits, cabi.mix_sketch_seed(bases[0], c0 + replay))
        assert torch.equal(y, ye) and torch.equal(state, state_e) and torch.equal(rstd, rstd_e)
        assert len(grads) == len(grads_e) and all(torch.equal(a, b) for a, b in zip(grads, grads_e))
        seen.append(grads[1].clone())
    assert not torch.equal(seen[0], seen[1])
