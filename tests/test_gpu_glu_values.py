"""The VALUES the kernels of the gated product see (fewbit_amd/csrc/fewbit_glu.hip): every gate a 16-bit format has, against a committed set of
ups, forward and -- through constant groups, which decode exactly -- backward; fp32 on probe patterns against ATen; and the value edges of the
packed form through the GLU kernels' own copies of its arithmetic.  The other GLU tests draw 3 N(0, 1): no gate beyond about +-13.

The bound is the unit's own (tests/test_gpu_glu.py): a 16-bit ``y``, ``d_up`` and rebuilt product lie within ``(h + 2^-20) |R| + the smallest
subnormal`` of the float64 result R, ``d_gate`` within the same with the 2^-20 taken of the magnitudes of the terms ``act'`` adds.  Near the
largest finite value ``max``: the bound applies and the result is finite while ``|R| < max (1 - 2 h)``; it is the infinity of R's sign where
``|R| > max (1 + 2 h)``; in between either is accepted, and that band is at most 0.1 % of the finite cases (asserted; the same figure is asserted
of the committed inputs alone in tests/test_glu_values_host.py).  The float64 formulas are glu_harness's ``act64``, ``slope64``, ``slope_terms64``.

MEASURED on an MI355X: EXPERIMENTS.md section 8.24 holds what each test prints."""
import functools

import pytest
import torch

from fewbit_amd import cabi_x
from glu_harness import (BACK_GY, BACK_UPS, FINITE_UPS, GATE_DOMAIN, INT16, UP_DOMAIN, UPS, act64, act_vanishes, decoded, exact_product, finite_patterns, fp32_gates, FP32_UPS, gate_up_grid, halves,
                         held, one_ulp_off, restated, slope64, slope_terms64, torch_act, ulp_error)
from norm_harness import DEV

pytestmark = pytest.mark.gpu

SIXTEEN = (torch.float16, torch.bfloat16)
DTYPES = (torch.float32, ) + SIXTEEN
ACTIVATIONS = ('silu', 'gelu')
BITS = (2, 4, 8)
SEED = 0x0fedcba987654321
ids = lambda d: str(d).split('.')[-1]
raw = lambda t: t.contiguous().view(-1).view(torch.uint8)


def off_by_one(t):
    """`t` (2-D) on the device, one element behind a 16-byte aligned address: the element path"""
    buffer = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
    view = buffer[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == t.element_size()
    return view


def worst_of(ok, half_ulps, gate, other, what):
    at = int(half_ulps.argmax())
    line = f'{what}: worst {float(half_ulps.view(-1)[at]):.4f} half ulps at gate {float(gate.reshape(-1)[at])!r}, {float(other.reshape(-1)[at])!r}'
    bad = (~ok).view(-1).nonzero().flatten()
    if bad.numel():
        line += f'; {bad.numel()} outside the bound, gates {float(gate.reshape(-1)[bad].min())!r} .. {float(gate.reshape(-1)[bad].max())!r}, first at ' + ', '.join(
            f'({float(gate.reshape(-1)[i])!r}, {float(other.reshape(-1)[i])!r})' for i in bad[:6].tolist())
    return line


# ---- 1. forward: all 65 536 gates x 24 ups ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def grid(dtype):
    return gate_up_grid(dtype)


@pytest.mark.parametrize('activation', ACTIVATIONS)
@pytest.mark.parametrize('dtype', SIXTEEN, ids=ids)
def test_the_forward_on_every_gate_of_the_format(dtype, activation):
    """65536 x 24: the vector path, the same from a base one element off (the element path), the plain forward; y against act64(gate) * up.
    What is printed is in EXPERIMENTS.md section 8.24."""
    gate, up = grid(dtype)
    gd, ud = gate.to(DEV), up.to(DEV)
    y, state = cabi_x.glu_forward(gd, ud, activation, 4, SEED)
    plain, none = cabi_x.glu_forward(gd, ud, activation, keep=False)
    moved = torch.zeros(y.numel() + 1, dtype=dtype, device=DEV)[1:].view(y.shape)
    cabi_x.glu_forward(off_by_one(gate), off_by_one(up), activation, 4, SEED, y=moved)
    plain_moved = torch.zeros(y.numel() + 1, dtype=dtype, device=DEV)[1:].view(y.shape)
    cabi_x.glu_forward(off_by_one(gate), off_by_one(up), activation, keep=False, y=plain_moved)
    assert none is None and torch.equal(raw(plain), raw(y)), 'the plain forward gives other bytes'
    assert torch.equal(raw(moved), raw(y)) and torch.equal(raw(plain_moved), raw(y)), 'the element path gives other bytes'
    y = y.cpu()
    exact = exact_product(gate, up, activation)
    vanishing = act_vanishes(gate, up, activation)
    ok, half_ulps, band = held(y, exact, dtype, vanishing=vanishing)
    finite = torch.isfinite(gate.float()) & torch.isfinite(up.float())
    assert int(finite.sum()) == finite_patterns(dtype).numel() * FINITE_UPS
    share = float(band.sum()) / float(finite.sum())
    print(f'\n{ids(dtype)} {activation} ' + worst_of(ok, half_ulps, gate, up, 'y'))
    print(f'{ids(dtype)} {activation} y: {one_ulp_off(y[finite], exact[finite], dtype)} of {int(finite.sum())} finite cases one ulp from the correctly rounded result; '
          f'band around the largest finite value {100 * share:.4f} %')
    assert share <= 0.001
    assert torch.equal(torch.isnan(y) & ~vanishing, torch.isnan(exact)), 'NaN in other places than float64'
    assert bool(ok.all()), worst_of(ok, half_ulps, gate, up, f'{ids(dtype)} {activation} y')


# ---- 2. backward on rows of one gate and one up: groups that decode exactly ----------------------------------------------------------------------------------
def back_gates(dtype, bits):
    """every finite gate at 4 bits; at 2 and 8 (the same decode, another word width) the gates with |g| >= 8 and every 64th pattern"""
    g = finite_patterns(dtype)
    if bits == 4:
        return g
    return g[(g.float().abs() >= 8) | (torch.arange(g.numel()) % 64 == 0)]


def constant_rows(t):
    """every row of a device tensor is 64 times one bit pattern -> column 0 on the host"""
    as_int = t.view(INT16)
    assert bool((as_int == as_int[:, :1]).all()), 'a row of constant inputs is not constant'
    return t[:, 0].cpu()


@pytest.mark.parametrize('bits', BITS)
@pytest.mark.parametrize('activation', ACTIVATIONS)
@pytest.mark.parametrize('dtype', SIXTEEN, ids=ids)
def test_the_backward_on_every_gate_through_groups_that_decode_exactly(dtype, activation, bits):
    """rows x 64 with one gate and one up per row: step 0, codes 0, g^ = g and u^ = u (a -0 decodes to +0), so act and act' are evaluated on known
    inputs.  Four calls: every gate meets four ups."""
    gates = back_gates(dtype, bits)
    rows = gates.numel()
    r = torch.arange(rows)
    lines, failures = [], []
    for call in range(4):
        ups = torch.tensor(BACK_UPS, dtype=torch.float64).to(dtype)[(r + call) % len(BACK_UPS)]
        gys = torch.tensor(BACK_GY, dtype=torch.float64).to(dtype)[(3 * r + call) % len(BACK_GY)]
        wide = lambda v: v[:, None].expand(rows, 64).contiguous()
        G, U, GY = wide(gates), wide(ups), wide(gys)
        y, state = cabi_x.glu_forward(G.to(DEV), U.to(DEV), activation, bits, SEED)
        assert torch.equal(state.cpu(), cabi_x.glu_state_host(G.float(), U.float(), SEED, bits)), f'call {call}: the state is not the host evaluation'
        d_gate, d_up = cabi_x.glu_backward(GY.to(DEV), state, activation, bits)
        d_gate2, d_up2, product = cabi_x.glu_backward_product(GY.to(DEV), state, activation, bits)
        assert torch.equal(raw(d_gate), raw(d_gate2)) and torch.equal(raw(d_up), raw(d_up2)), 'glu_backward and glu_backward_product differ'
        assert bool((product == y).all()), 'the rebuilt product is not the forward y on exact decodes'
        y, d_gate, d_up, product = (constant_rows(t) for t in (y, d_gate, d_up, product))
        g_hat = gates.double() + 0.0                                                   # the decode of -0 is +0
        act, pair = act64(g_hat, activation), gys.double() * ups.double()
        checks = (('d_up', d_up, gys.double() * act, None, gys), ('product', product, act * ups.double(), None, ups),
                  ('d_gate beyond 2^-20 of its terms', d_gate, pair * slope64(g_hat, activation), pair.abs() * slope_terms64(g_hat, activation), ups))
        for name, got, exact, scale, other in checks:
            ok, half_ulps, band = held(got, exact, dtype, scale)
            line = f'{ids(dtype)} {activation} bits {bits} call {call} ' + worst_of(ok, half_ulps, gates, other, name)
            lines.append(line)
            if not bool(ok.all()):
                failures.append(line)
    print('\n' + '\n'.join(lines))
    assert not failures, '\n'.join(failures)


# ---- 3. fp32 on probe patterns, against ATen -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('activation', ACTIVATIONS)
def test_fp32_on_probe_patterns_against_aten(activation):
    """the project's convention for fp32: the largest error in ulps is at most that of torch's own fp32 act(g) * u on the same tensors, plus 2.
    Taken over the cases whose float64 result is finite and inside fp32's range, over all gates and over the gates above -5 (below, ATen's gelu
    and ours are both 0 where erf rounds to -1, and the maximum is that collapse)."""
    g = fp32_gates()
    rows = g.numel()
    gate = g[:, None].expand(rows, len(FP32_UPS)).contiguous()
    up = torch.tensor(FP32_UPS, dtype=torch.float32)[None, :].expand(rows, len(FP32_UPS)).contiguous()
    y, _ = cabi_x.glu_forward(gate.to(DEV), up.to(DEV), activation, 4, SEED)
    moved = torch.zeros(y.numel() + 1, dtype=torch.float32, device=DEV)[1:].view(y.shape)
    cabi_x.glu_forward(off_by_one(gate), off_by_one(up), activation, keep=False, y=moved)
    assert torch.equal(raw(moved), raw(y))
    y, theirs = y.cpu(), (torch_act(gate.to(DEV), activation) * up.to(DEV)).cpu()
    exact = exact_product(gate, up, activation)
    inside = torch.isfinite(exact) & (exact.abs() < 3.0e38)
    assert torch.equal(torch.isnan(y), torch.isnan(exact)), 'NaN in other places than float64'
    for name, where in (('all gates', inside), ('gates above -5', inside & (gate > -5))):
        ours, torchs = ulp_error(y, exact)[where], ulp_error(theirs, exact)[where]
        print(f'\nfp32 {activation} {name}: max error {float(ours.max()):.2f} ulp, torch {float(torchs.max()):.2f} ulp')
        assert float(ours.max()) <= float(torchs.max()) + 2.0, name
    # recorded, not asserted: a zero where fp32 has a number for the result (u = 1)
    first = exact[:, 0]
    for who, got in (('ours', y[:, 0]), ("torch's", theirs[:, 0])):
        lost = (got == 0) & (first.abs() >= 2.0**-149) & torch.isfinite(first)
        span = f'gates {float(g[lost].min())!r} .. {float(g[lost].max())!r}, |result| up to {float(first[lost].abs().max()):.3e}' if bool(lost.any()) else 'nowhere'
        print(f'fp32 {activation}: {who} gives 0 for a representable result at {int(lost.sum())} of {rows} gates: {span}')


# ---- 4. the value edges of the packed form through the GLU kernels' own group_params / code_word / store_word ------------------------------------------
EDGES = ('overflow', 'constant', 'zeros', 'tiny')


def edge(clean, name, dtype):
    """`clean` with the case of tests/test_gpu_quant.py::test_poisoned_constant_and_tiny_groups_on_the_device in group 1 (flat elements 64 .. 127)"""
    fi, x = torch.finfo(dtype), clean.clone().view(-1)
    if name == 'overflow':
        x[64], x[127] = fi.max, -fi.max                               # fp32 / bf16: the range is not finite; fp16: it is, and the group is clean
    elif name == 'constant':
        x[64:128] = 0.3
    elif name == 'zeros':
        x[64:128] = 0.0
        x[64:128:3] = -0.0
    else:
        x[64:128] = (torch.arange(64) % 5).to(dtype) * fi.smallest_normal * fi.eps
    return x.view(clean.shape)


@pytest.mark.parametrize('bits', BITS)
@pytest.mark.parametrize('dtype', DTYPES, ids=ids)
def test_overflowing_constant_zero_and_denormal_groups_through_the_glu_kernels(dtype, bits):
    """3 x 56 (three groups, the last one short): one case in group 1 of gate, ANOTHER in group 1 of up; the vector path and a base one element off"""
    rows, width = 3, 56
    n = rows * width
    gen = torch.Generator().manual_seed(77)
    clean_g, clean_u, gy = ((3 * torch.randn(rows, width, generator=gen)).to(dtype) for _ in range(3))
    in_group = ((torch.arange(n) // 64) == 1).view(rows, width)
    for i, (case_g, activation) in enumerate(zip(EDGES, ('silu', 'gelu', 'silu', 'gelu'))):
        case_u = EDGES[(i + 1) % len(EDGES)]
        what = f'{ids(dtype)} bits {bits} {activation} gate {case_g} up {case_u}'
        gate, up = edge(clean_g, case_g, dtype), edge(clean_u, case_u, dtype)
        host = cabi_x.glu_state_host(gate.float(), up.float(), SEED, bits)
        part_g, part_u, zeros = halves(host, n, bits)
        assert torch.equal(part_g, torch.from_numpy(restated(gate.float().view(-1).numpy(), bits, SEED, GATE_DOMAIN).copy())), what
        assert torch.equal(part_u, torch.from_numpy(restated(up.float().view(-1).numpy(), bits, SEED, UP_DOMAIN).copy())), what
        assert not bool(zeros.any()), what
        outs = []
        for place in (lambda t: t.to(DEV), off_by_one):
            y, state = cabi_x.glu_forward(place(gate), place(up), activation, bits, SEED)
            assert torch.equal(state.cpu(), host), (what, torch.nonzero(state.cpu() != host)[:8].flatten().tolist())
            outs.append((y, ) + cabi_x.glu_backward(gy.to(DEV), state, activation, bits))
        assert all(torch.equal(raw(a), raw(b)) for a, b in zip(*outs)), what + ': the element path gives other bytes'
        y, d_gate, d_up = (t.cpu() for t in outs[0])
        # y: the exact forward, whatever the groups hold
        exact = exact_product(gate, up, activation)
        assert torch.equal(torch.isnan(y), torch.isnan(exact)), what
        if dtype == torch.float32:
            theirs = (torch_act(gate.to(DEV), activation) * up.to(DEV)).cpu()
            inside = torch.isfinite(exact) & (exact.abs() < 3.0e38)
            assert float(ulp_error(y, exact)[inside].max()) <= float(ulp_error(theirs, exact)[inside].max()) + 2.0, what
            assert bool((y[exact == 0] == 0).all()) and torch.equal(torch.signbit(y[exact == 0]), torch.signbit(exact[exact == 0])), what
        else:
            ok, half_ulps, _ = held(y, exact, dtype)
            assert bool(ok.all()), worst_of(ok, half_ulps, gate, up, what + ' y')
        # the gradients: NaN on exactly the 64 elements of a poisoned group, elsewhere to the bit those of ordinary values in that group
        poisoned = 'overflow' in (case_g, case_u) and dtype != torch.float16
        want_nan = in_group if poisoned else torch.zeros_like(in_group)
        assert torch.equal(torch.isnan(d_gate), want_nan) and torch.equal(torch.isnan(d_up), want_nan), what
        _, tame_state = cabi_x.glu_forward(clean_g.to(DEV), clean_u.to(DEV), activation, bits, SEED)
        tame_gate, tame_up = cabi_x.glu_backward(gy.to(DEV), tame_state, activation, bits)
        assert torch.equal(raw(d_gate[~in_group]), raw(tame_gate.cpu()[~in_group])) and torch.equal(raw(d_up[~in_group]), raw(tame_up.cpu()[~in_group])), what
        if not poisoned:
            # group 1 itself: the float64 formulas on the host decode
            gq, uq = (t.view(rows, width) for t in decoded(host, n, bits))
            pair = gy.double() * uq.double()
            ok, half_ulps, _ = held(d_gate, pair * slope64(gq, activation), dtype, pair.abs() * slope_terms64(gq, activation))
            assert bool(ok[in_group].all()), worst_of(ok, half_ulps, gq, uq, what + ' d_gate')
            want_up = gy.double() * act64(gq, activation)
            if dtype == torch.float32:
                theirs = gy * torch_act(gq.to(DEV), activation).cpu()
                assert float(ulp_error(d_up, want_up)[in_group].max()) <= float(ulp_error(theirs, want_up)[in_group].max()) + 2.0, what
            else:
                ok, half_ulps, _ = held(d_up, want_up, dtype)
                assert bool(ok[in_group].all()), worst_of(ok, half_ulps, gq, gy, what + ' d_up')
