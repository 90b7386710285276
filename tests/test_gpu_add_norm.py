"""The fused entry points of the companion library on the GPU (include/fewbit_hipx.h, "The sum of a seed in front of the norm";
fewbit_amd/csrc/fewbit_norm.hip), both kinds.  Everything is compared BIT FOR BIT (byte views, so a NaN equals itself) with what the library already
has, because the definition is the existing arithmetic in the existing order:

* forward: ``h`` is ``cabi_x.dropout_apply(x, seed, p, addend=residual)`` (torch's ``x + residual`` without a mask); ``y``, ``rstd``, the state and
  ``xhat`` are the plain ``*_norm_forward(h, ..., seed)``; without ``h_out`` and with ``keep=False`` the remaining outputs keep their bytes;
* backward from that state: ``dres`` is the plain ``dx`` without ``gh``; with it ``dx + gh`` by torch in fp32, and for 16-bit inputs
  ``(dx32 + gh.float()).to(dtype)`` with ``dx32`` the plain fp32 entry point on the widened ``gy`` and ``gamma`` (the plan is a function of the
  width only, so that is the same arithmetic); ``dbranch`` is ``dropout_apply(dres, seed, p)``; the sums are the plain backward's bytes;
* guard bytes intact, inputs unchanged, two runs byte-equal, NULL outputs skipped and without the sums the workspace untouched.

Widths: with a mask every plan threshold and the next multiple of 8; without one also the ragged widths around them.  A workgroup that walks several
tiles: widths 8 and 520, and -- with ``norm_harness.walk`` and the tables of tests/test_gpu_norm.py -- backward every lanes-per-row from 16 to 1024,
forward 256 lanes per row with 1, 2 and 4 blocks per lane, each with a mask."""
import itertools

import pytest
import torch

from fewbit_amd import cabi_x
from norm_harness import DEV, EPS, FILL, SEED, Guarded, first_difference, options, seed_argument, tiled, walks

pytestmark = pytest.mark.gpu
MASKED_WIDTHS = (8, 64, 72, 128, 136, 512, 520, 768, 1024, 1032, 2048, 2056, 4096, 4104, 8192)
RAGGED_WIDTHS = (1, 7, 9, 63, 65, 129, 513, 770, 1025, 2049, 4097)
ROWS = (1, 3, 37)
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
BITS = (2, 4, 8)
KINDS = {'layer': (cabi_x.add_layer_norm_forward, cabi_x.add_layer_norm_backward, cabi_x.layer_norm_forward, cabi_x.layer_norm_backward, True),
         'rms': (cabi_x.add_rms_norm_forward, cabi_x.add_rms_norm_backward, cabi_x.rms_norm_forward, cabi_x.rms_norm_backward, False)}
ids = lambda d: str(d).split('.')[-1] if isinstance(d, torch.dtype) else None
same = lambda a, b: a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def cases():
    """(index, width, rows, p): every masked width with p = 0.1, 0.5 and 0 in turn over its three row counts, every ragged width without a mask"""
    for i, (width, rows) in enumerate(itertools.product(MASKED_WIDTHS + RAGGED_WIDTHS, ROWS)):
        yield i, width, rows, (0.1, 0.5, 0.0)[(i + i // 3) % 3] if width in MASKED_WIDTHS else 0.0


def inputs(rows, width, dtype, centred, affine=True, salt=0):
    g = torch.Generator().manual_seed(1000 * width + rows + salt)
    x = torch.randn(rows, width, generator=g).to(dtype)
    res = (3 + 2 * torch.randn(rows, width, generator=g)).to(dtype)
    parameters = ((1 + 0.5 * torch.randn(width, generator=g)).to(dtype), ) + ((torch.randn(width, generator=g).to(dtype), ) if centred else ())
    gy, gh = torch.randn(rows, width, generator=g).to(dtype), torch.randn(rows, width, generator=g).to(dtype)
    return x, res, parameters if affine else (None, ) * len(parameters), gy, gh


def run_forward(kind, x, res, parameters, bits, seed, p, off, keep=True, want_h=True, want_xhat=True):
    """the fused call into guarded buffers -> (y, h, rstd, state, xhat) as tensors (None where not asked for) after guards and inputs were checked"""
    rows, width = x.shape
    gx, gr = Guarded(x.numel(), x.dtype, off, x), Guarded(x.numel(), x.dtype, off, res)
    gp = tuple(None if t is None else Guarded(width, x.dtype, off, t) for t in parameters)
    y, rstd = Guarded(x.numel(), x.dtype, off), Guarded(rows, torch.float32, off)
    h = Guarded(x.numel(), x.dtype, off) if want_h else None
    state = Guarded(cabi_x.norm_state_bytes(rows, width, bits), torch.uint8, 8 * off) if keep else None
    xhat = Guarded(x.numel(), torch.float32, off) if want_xhat else None
    view = lambda b: None if b is None else b.t.view(rows, width)
    KINDS[kind][0](view(gx), view(gr), *(None if b is None else b.t for b in gp), EPS, p, bits, seed, keep=keep, y=view(y), h=view(h), rstd=rstd.t,
                   state=None if state is None else state.t, xhat=view(xhat))
    torch.cuda.synchronize()
    for name, buffer in (('y', y), ('h', h), ('rstd', rstd), ('state', state), ('xhat', xhat)):
        assert buffer is None or buffer.intact(), f'{name}: guard bytes were written'
    for name, buffer in (('x', gx), ('residual', gr), ('gamma', gp[0]), ('beta', gp[-1])):
        assert buffer is None or buffer.unchanged(), f'{name} was written'
    return view(y), view(h), rstd.t, None if state is None else state.t, view(xhat)


def composed_forward(kind, x, res, parameters, bits, seed, p):
    """(y, h, rstd, state, xhat) of the two existing calls with the one seed"""
    x, res = x.to(DEV), res.to(DEV)
    h = cabi_x.dropout_apply(x, seed, p, addend=res) if cabi_x.dropout_threshold(p) else x + res
    y, rstd, state, xhat = KINDS[kind][2](h, *(None if t is None else t.to(DEV) for t in parameters), EPS, bits, seed, want_xhat=True)
    return y, h, rstd, state, xhat


def run_backward(kind, gy, gh, state, rstd, gamma, bits, seed, p, off, want, workspace=None):
    """the fused call into guarded buffers -> (dres, dbranch, dgamma[, dbeta]) as tensors (None where not wanted)"""
    rows, width = gy.shape
    g_gy, g_state, g_rstd = Guarded(gy.numel(), gy.dtype, off, gy), Guarded(state.numel(), torch.uint8, 8 * off, state), Guarded(rows, torch.float32, off, rstd)
    g_gh = None if gh is None else Guarded(gy.numel(), gy.dtype, off, gh)
    g_gamma = None if gamma is None else Guarded(width, gy.dtype, off, gamma)
    sizes = ((gy.numel(), gy.dtype), (gy.numel(), gy.dtype), (width, torch.float32), (width, torch.float32))
    outs = [Guarded(*size, off) if wanted else None for size, wanted in zip(sizes, want)]
    views = tuple(None if b is None else (b.t.view(rows, width) if j < 2 else b.t) for j, b in enumerate(outs))
    names = ('dres', 'dbranch', 'dgamma', 'dbeta')[:len(want)]
    KINDS[kind][1](g_gy.t.view(rows, width), g_state.t, g_rstd.t, None if g_gamma is None else g_gamma.t, bits, seed, p,
                   None if g_gh is None else g_gh.t.view(rows, width), tuple(want), workspace=workspace, **dict(zip(names, views)))
    torch.cuda.synchronize()
    for name, buffer in zip(names, outs):
        assert buffer is None or buffer.intact(), f'{name}: guard bytes were written'
    for name, buffer in (('gy', g_gy), ('gh', g_gh), ('state', g_state), ('rstd', g_rstd), ('gamma', g_gamma)):
        assert buffer is None or buffer.unchanged(), f'{name} was written'
    return views


def composed_backward(kind, gy, gh, state, rstd, gamma, bits, seed, p):
    """(dres, dbranch, dgamma[, dbeta]) from the plain backward, torch's add and the dropout's own backward"""
    plain = KINDS[kind][3]
    gy, gamma = gy.to(DEV), None if gamma is None else gamma.to(DEV)
    dx, *sums = plain(gy, state, rstd, gamma, bits)
    if gh is None:
        dres = dx
    elif gy.dtype == torch.float32:
        dres = dx + gh.to(DEV)
    else:
        dx32 = plain(gy.float(), state, rstd, None if gamma is None else gamma.float(), bits, (True, ) + (False, ) * len(sums))[0]
        dres = (dx32 + gh.to(DEV).float()).to(gy.dtype)
    dbranch = cabi_x.dropout_apply(dres, seed, p) if cabi_x.dropout_threshold(p) else None
    return (dres, dbranch, *sums)


@pytest.mark.parametrize('bits', BITS)
@pytest.mark.parametrize('dtype', DTYPES, ids=ids)
@pytest.mark.parametrize('kind', KINDS)
def test_forward_is_the_dropout_add_then_the_plain_norm_bit_for_bit(kind, dtype, bits):
    centred = KINDS[kind][4]
    for i, width, rows, p in cases():
        off, affine, device_word = options(i)
        x, res, parameters, _, _ = inputs(rows, width, dtype, centred, affine)
        label = f'{rows} x {width} p {p} off {off} affine {affine} device word {device_word}'
        got = run_forward(kind, x, res, parameters, bits, seed_argument(device_word), p, off)
        want = composed_forward(kind, x, res, parameters, bits, SEED, p)
        for name, a, b in zip(('y', 'h', 'rstd', 'state', 'xhat'), got, want):
            assert same(a, b), f'{label}: {name} differs'
        # without h_out, and the plain forward that keeps nothing: the remaining outputs keep their bytes
        y, h, rstd, state, xhat = run_forward(kind, x, res, parameters, bits, SEED, p, off, want_h=False)
        assert h is None and all(same(a, b) for a, b in zip((y, rstd, state, xhat), (got[0], *got[2:]))), label
        y, h, rstd, state, _ = run_forward(kind, x, res, parameters, bits, SEED, p, off, keep=False, want_xhat=False)
        assert state is None and same(y, got[0]) and same(h, got[1]) and same(rstd, got[2]), label
        again = run_forward(kind, x, res, parameters, bits, SEED, p, off)
        assert all(same(a, b) for a, b in zip(again, got)), f'{label}: two runs differ'


@pytest.mark.parametrize('bits', BITS)
@pytest.mark.parametrize('dtype', DTYPES, ids=ids)
@pytest.mark.parametrize('kind', KINDS)
def test_backward_is_the_plain_backward_the_add_and_the_dropout_bit_for_bit(kind, dtype, bits):
    centred = KINDS[kind][4]
    sums = 2 if centred else 1
    for i, width, rows, p in cases():
        off, affine, device_word = options(i)
        mask = cabi_x.dropout_threshold(p) > 0
        x, res, parameters, gy, gh = inputs(rows, width, dtype, centred, affine)
        label = f'{rows} x {width} p {p} off {off} affine {affine} device word {device_word}'
        _, _, rstd, state, _ = composed_forward(kind, x, res, parameters, bits, SEED, p)
        gamma = parameters[0]
        everything = (True, mask) + (True, ) * sums
        got = run_backward(kind, gy, gh, state, rstd, gamma, bits, seed_argument(device_word), p, off, everything)
        want = composed_backward(kind, gy, gh, state, rstd, gamma, bits, SEED, p)
        for name, a, b in zip(('dres', 'dbranch', 'dgamma', 'dbeta'), got, want):
            assert (a is None and b is None) or same(a, b), f'{label}: {name} differs'
        again = run_backward(kind, gy, gh, state, rstd, gamma, bits, SEED, p, off, everything)
        assert all((a is None and b is None) or same(a, b) for a, b in zip(again, got)), f'{label}: two runs differ'
        # no gradient arrives at h: dres is the plain dx
        bare = run_backward(kind, gy, None, state, rstd, gamma, bits, SEED, p, off, everything)
        want = composed_backward(kind, gy, None, state, rstd, gamma, bits, SEED, p)
        assert all((a is None and b is None) or same(a, b) for a, b in zip(bare, want)), f'{label}: without gh'
        # NULL outputs are skipped: the others keep their bytes, and without the sums the workspace is not touched
        scratch = torch.full((cabi_x.norm_workspace_bytes(rows, width), ), FILL, dtype=torch.uint8, device=DEV)
        only = run_backward(kind, gy, gh, state, rstd, gamma, bits, SEED, p, off, (not mask, mask) + (False, ) * sums, scratch)
        assert same(only[1] if mask else only[0], got[1] if mask else got[0]) and all(t is None for t in only[2:]) and bool((scratch == FILL).all()), label
        only = run_backward(kind, gy, gh, state, rstd, gamma, bits, SEED, p, off, (mask, False) + (True, ) * sums)
        assert (not mask or same(only[0], got[0])) and all(same(a, b) for a, b in zip(only[2:], got[2:])), label


# ---- a workgroup that walks several tiles ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows, width', ((2 * 16384 * 2 + 1, 520), (2 * 16384 * 32 + 5, 8)), ids=('width_520_through_the_lds_slots', 'width_8'))
def test_forward_a_workgroup_walks_on(rows, width):
    """width 520: 128 lanes per row, 2 rows per tile, ONE row sum per tile (the RMS kind) whose LDS slots alternate; width 8: 32 rows per tile.  Each
    one row or five past two full sweeps of the 16384 workgroups"""
    kind, dtype, bits, p = 'rms', torch.bfloat16, 4, 0.1
    x, res, parameters, _, _ = inputs(rows, width, dtype, False)
    got = run_forward(kind, x, res, parameters, bits, SEED, p, 0)
    want = composed_forward(kind, x, res, parameters, bits, SEED, p)
    for name, a, b in zip(('y', 'h', 'rstd', 'state', 'xhat'), got, want):
        assert same(a, b), f'{name} differs'


@pytest.mark.parametrize('rows', (2 * 512 * 8 + 5, 3 * 512 * 8), ids=('a_third_tile_begun', 'three_full_tiles'))
def test_backward_width_520_a_workgroup_walks_on(rows):
    """128 lanes per row, 8 rows per tile, 512 workgroups: every workgroup walks two tiles and some (or all) a third"""
    kind, dtype, bits, p, width = 'layer', torch.float16, 2, 0.5, 520
    x, res, parameters, gy, gh = inputs(rows, width, dtype, True)
    _, _, rstd, state, _ = composed_forward(kind, x, res, parameters, bits, SEED, p)
    got = run_backward(kind, gy, gh, state, rstd, parameters[0], bits, SEED, p, 0, (True, True, True, True))
    want = composed_backward(kind, gy, gh, state, rstd, parameters[0], bits, SEED, p)
    for name, a, b in zip(('dres', 'dbranch', 'dgamma', 'dbeta'), got, want):
        assert same(a, b), f'{name} differs'


def mismatch(got, want, names, row_bytes):
    """'' when every output has the bytes it should have, else the first output that does not and where"""
    for name, a, b in zip(names, got, want):
        if not ((a is None and b is None) or same(a, b)):
            return f'{name}: {first_difference(a, b, row_bytes(a))}'
    return ''


def tiled_inputs(case, rows, centred):
    """`inputs` of 37 rows repeated on the GPU (the masks and the rounding bits still differ from row to row: they come from the flat index)"""
    x, res, parameters, gy, gh = inputs(37, case.width, case.dtype, centred, case.affine)
    return (*(tiled(t, rows)[0] for t in (x, res)), parameters, *(tiled(t, rows)[0] for t in (gy, gh)))


@pytest.mark.parametrize('kind, case', [(kind, case) for shift, kind in enumerate(KINDS) for case in walks('forward', shift, fused=True)], ids=str)
def test_forward_a_workgroup_walks_on_at_256_lanes_per_row_and_1_2_4_blocks_per_lane(kind, case):
    """one row past one or two sweeps of the 16384 workgroups with a mask, where a lane holds 1, 2 or 4 blocks: the composition, bit for bit"""
    rows, p = case.rows('forward'), (0.1, 0.5)[case.bits == 4]
    x, res, parameters, _, _ = tiled_inputs(case, rows, KINDS[kind][4])
    got = run_forward(kind, x, res, parameters, case.bits, SEED, p, case.off)
    want = composed_forward(kind, x, res, parameters, case.bits, SEED, p)
    wrong = mismatch(got, want, ('y', 'h', 'rstd', 'state', 'xhat'), lambda t: t[0].numel() * t.element_size() if t.dim() == 2 else None)
    assert not wrong, f'{kind} {rows} x {case.width} ({case}) p {p}: {wrong}'


@pytest.mark.parametrize('kind, case', [(kind, case) for shift, kind in enumerate(KINDS) for case in walks('backward', shift, fused=True)], ids=str)
def test_backward_a_workgroup_walks_on_at_every_lanes_per_row(kind, case):
    """16 to 1024 lanes per row (norm_harness.walk asserts the 512 workgroups from the workspace query), one row past one and two sweeps and three
    full sweeps, with gh, a mask and every output: the composition, bit for bit"""
    rows, p = case.rows('backward'), (0.1, 0.5)[case.bits == 4]
    centred = KINDS[kind][4]
    x, res, parameters, gy, gh = tiled_inputs(case, rows, centred)
    _, _, rstd, state, _ = composed_forward(kind, x, res, parameters, case.bits, SEED, p)
    names = ('dres', 'dbranch', 'dgamma', 'dbeta')[:4 if centred else 3]
    got = run_backward(kind, gy, gh, state, rstd, parameters[0], case.bits, SEED, p, case.off, (True, ) * len(names))
    want = composed_backward(kind, gy, gh, state, rstd, parameters[0], case.bits, SEED, p)
    wrong = mismatch(got, want, names, lambda t: t[0].numel() * t.element_size() if t.dim() == 2 else None)
    assert not wrong, f'{kind} {rows} x {case.width} ({case}) p {p}: {wrong}'


# ---- non-finite inputs -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('poison', ('nan', 'inf'))
@pytest.mark.parametrize('kind', KINDS)
def test_a_dropped_non_finite_element_is_gone_and_a_kept_one_poisons_as_the_plain_kernel_does(kind, poison):
    rows, width, bits, p, dtype = 5, 200, 4, 0.5, torch.bfloat16
    x, res, parameters, _, _ = inputs(rows, width, dtype, KINDS[kind][4], salt=3)
    keep = cabi_x.dropout_keep(SEED, rows * width, p).view(rows, width)
    dropped, kept = int(torch.nonzero(~keep[2])[0]), int(torch.nonzero(keep[2])[0])
    clean = run_forward(kind, x, res, parameters, bits, SEED, p, 0)
    gone = x.clone()
    gone[2, dropped] = float(poison)
    got = run_forward(kind, gone, res, parameters, bits, SEED, p, 0)
    assert all(same(a, b) for a, b in zip(got, clean))                    # the element has no influence at all
    assert same(got[1][2, dropped].cpu().reshape(1), res[2, dropped].reshape(1)) and bool(torch.isfinite(got[0][2]).all())
    hit = x.clone()
    hit[2, kept] = float(poison)
    got = run_forward(kind, hit, res, parameters, bits, SEED, p, 0)
    want = composed_forward(kind, hit, res, parameters, bits, SEED, p)
    assert all(same(a, b) for a, b in zip(got, want)) and not bool(torch.isfinite(got[1][2, kept]))
    assert bool(torch.isnan(got[0][2]).any())
    others = [0, 1, 3, 4]
    assert all(same(a[others], b[others]) for a, b in zip((got[0], got[1], got[2], got[4]), (clean[0], clean[1], clean[2], clean[4])))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_what_is_refused_is_refused_before_anything_is_written(kind):
    forward, backward, _, _, centred = KINDS[kind]
    rows, width, bits, dtype = 3, 770, 4, torch.bfloat16
    x, res, parameters, gy, gh = inputs(rows, width, dtype, centred)
    x, res, gy = x.to(DEV), res.to(DEV), gy.to(DEV)
    parameters = tuple(t.to(DEV) for t in parameters)
    filled = lambda dt, *shape: torch.full((torch.Size(shape).numel() * torch.empty(0, dtype=dt).element_size(), ), FILL, dtype=torch.uint8, device=DEV).view(dt).view(shape)
    y, h, rstd, state = filled(dtype, rows, width), filled(dtype, rows, width), filled(torch.float32, rows), filled(torch.uint8, cabi_x.norm_state_bytes(rows, width, bits))
    untouched = lambda *ts: all(bool((t.view(torch.uint8) == FILL).all()) for t in ts)
    # a mask at a width that is no multiple of 8: FEWBIT_ERR_UNSUPPORTED
    with pytest.raises(cabi_x.FewbitHipError, match=r'error -2: .*multiple of 8'):
        forward(x, res, *parameters, EPS, 0.1, bits, SEED, y=y, h=h, rstd=rstd, state=state)
    torch.cuda.synchronize()
    assert untouched(y, h, rstd, state)
    _, _, rstd_ok, state_ok, _ = forward(x, res, *parameters, EPS, 0.0, bits, SEED)            # without a mask the width is served
    dres, dbranch = filled(dtype, rows, width), filled(dtype, rows, width)
    with pytest.raises(cabi_x.FewbitHipError, match=r'error -2: .*multiple of 8'):
        backward(gy, state_ok, rstd_ok, parameters[0], bits, SEED, 0.1, dres=dres, dbranch=dbranch)
    # dbranch without a mask, and a threshold that drops everything
    with pytest.raises(cabi_x.FewbitHipError, match=r'error -1: .*dbranch'):
        backward(gy, state_ok, rstd_ok, parameters[0], bits, SEED, 0.0, want=(True, True) + (True, ) * (2 if centred else 1), dres=dres, dbranch=dbranch)
    with pytest.raises(cabi_x.FewbitHipError, match=r'error -1: .*threshold = 65536'):
        forward(x, res, *parameters, EPS, 1.0, bits, SEED, y=y, h=h, rstd=rstd, state=state)
    with pytest.raises(cabi_x.FewbitHipError, match=r'error -1: .*threshold = 65536'):
        backward(gy, state_ok, rstd_ok, parameters[0], bits, SEED, 1.0, dres=dres, dbranch=dbranch)
    torch.cuda.synchronize()
    assert untouched(y, h, rstd, state, dres, dbranch)
