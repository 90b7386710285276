"""Column sampling of LinearCRS on the gfx950 kernels of fewbit_amd/csrc/fewbit_crs.hip (companion library: fewbit_hipx_crs_gather,
fewbit_hipx_crs_scatter): both entry points bit for bit against the torch formulation with the columns the HOST evaluates for the same seed
(cabi_x.crs_columns), and the layer's contract -- reproducible from torch.manual_seed, no synchronisation, capture into a hipGraph with
fresh columns on every replay, the PyTorch formulation for everything the kernels do not take."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fewbit
from fewbit_amd import cabi_x, linear
from helpers import GOLDEN

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}


@pytest.fixture(autouse=True)
def native_sketch_on():
    prev = linear.use_native_sketch(True)
    yield
    linear.use_native_sketch(prev)


@pytest.fixture(scope='module')
def lref():
    with np.load(GOLDEN / 'linear_ref.npz') as z:
        return {k: torch.from_numpy(z[k].copy()) for k in z.files if z[k].dtype.kind in 'fiu'}


def bits(t):
    return t.contiguous().view(BITS[t.dtype])


def guarded(rows, cols, dtype, offset, ld=None):
    """-> (NaN-filled flat buffer, rows x cols view of it `offset` elements in, rows `ld` apart): what lies around the view must stay NaN"""
    ld = cols if ld is None else ld
    flat = torch.full((2 * offset + rows * ld, ), float('nan'), dtype=dtype, device=DEV)
    return flat, flat[offset:offset + rows * ld].view(rows, ld)[:, :cols]


def columns(seed, in_features, nopairs):
    """-> (cols on the device, fp32 scale on the device, m) from the host evaluation of the seed"""
    cols, count = cabi_x.crs_columns(seed, in_features, nopairs)
    scale = (count.double() * in_features / nopairs).float()
    return cols.to(DEV), scale.to(DEV), cols.numel()


# rows, in_features, ld, nopairs, columns beyond m (None: cap = min(nopairs, in_features)), offset of out in its guard buffer (elements)
GATHER_CASES = [
    (5, 770, 770, 385, 0, 64),          # a ragged in_features
    (16, 768, 800, 384, 0, 61),         # ld > in_features; out starts off a 16-byte boundary
    (1, 3072, 3072, 1536, 0, 64),       # a single row
    (33, 770, 776, 385, None, 61),      # cap > m: what a captured layer keeps
    (19, 768, 768, 384, 3, 64),
    (7, 16384, 16384, 8192, 5, 3),      # past the LDS counters of the prep kernel: counted with global atomics
    (3, 7, 9, 30, None, 1),             # more draws than columns
    (40, 3072, 3072, 1, 0, 2),          # one draw
]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', GATHER_CASES)
def test_gather_is_the_torch_formulation_bit_for_bit(dtype, case):
    rows, in_features, ld, nopairs, extra, offset = case
    seed = 0x5eed0000 + rows * 131 + in_features
    cols, scale, m = columns(seed, in_features, nopairs)
    cap = min(nopairs, in_features) if extra is None else min(m + extra, min(nopairs, in_features))
    xbuf, x = guarded(rows, in_features, dtype, 8, ld)
    x.copy_(torch.randn(rows, in_features, generator=torch.Generator().manual_seed(rows)).to(dtype))
    obuf, out = guarded(rows, cap, dtype, offset)
    got = cabi_x.crs_gather(x, seed, nopairs, cap, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and got.shape == (rows, cap)
    want = (x.float()[:, cols] * scale).to(dtype)
    assert torch.equal(bits(out[:, :m]), bits(want))
    assert not bool(bits(out[:, m:]).any())                   # exactly +0
    assert torch.isnan(obuf[:offset]).all() and torch.isnan(obuf[offset + rows * cap:]).all()      # around out: untouched
    pad = xbuf[8:8 + rows * ld].view(rows, ld)[:, in_features:]
    assert torch.isnan(pad).all() and torch.isnan(xbuf[:8]).all() and torch.isnan(xbuf[8 + rows * ld:]).all()
    # the seed as a device word: the same columns, cap defaults to min(nopairs, in_features)
    word = torch.tensor([seed], dtype=torch.int64, device=DEV)
    wide = cabi_x.crs_gather(x, word, nopairs)
    assert wide.shape == (rows, min(nopairs, in_features))
    assert torch.equal(bits(wide[:, :m]), bits(want)) and not bool(bits(wide[:, m:]).any())
    # an eager call sizes itself: cap defaults to m
    assert torch.equal(bits(cabi_x.crs_gather(x, seed, nopairs)), bits(want))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', [(4, 770, 385, 0, 64), (48, 768, 384, None, 61), (1, 3072, 1536, 3, 64), (9, 16384, 8192, 0, 3), (5, 7, 30, None, 1),
                                  (130, 773, 400, 2, 5)])
def test_scatter_writes_the_whole_weight_gradient_bit_for_bit(dtype, case):
    out_features, in_features, nopairs, extra, offset = case
    seed = 0xc0150000 + out_features * 131 + in_features
    cols, _, m = columns(seed, in_features, nopairs)
    cap = min(nopairs, in_features) if extra is None else min(m + extra, min(nopairs, in_features))
    t = torch.randn(out_features, cap, generator=torch.Generator().manual_seed(cap)).to(dtype).to(DEV)
    t[0, 0] = -0.0                                                                      # (the bits of t are copied)
    gbuf, gw = guarded(out_features, in_features, dtype, offset)
    got = cabi_x.crs_scatter(t, seed, in_features, nopairs, out=gw)
    torch.cuda.synchronize()
    assert got.data_ptr() == gw.data_ptr()
    assert not torch.isnan(gw).any()                                                    # NaN-filled before: fully overwritten
    assert torch.equal(bits(gw[:, cols]), bits(t[:, :m]))
    rest = torch.ones(in_features, dtype=torch.bool, device=DEV)
    rest[cols] = False
    assert not bool(bits(gw[:, rest]).any())        # every other entry: +0.0
    assert torch.isnan(gbuf[:offset]).all() and torch.isnan(gbuf[offset + out_features * in_features:]).all()
    word = torch.tensor([seed], dtype=torch.int64, device=DEV)
    assert torch.equal(bits(cabi_x.crs_scatter(t, word, in_features, nopairs)), bits(gw))


def torch_formulation(x, w, b, gy, seed, nopairs):
    """the layer's PyTorch formulation with the columns of `seed`: -> (y, gx, gw, gb)"""
    in_features = w.shape[1]
    cols, scale, _ = columns(seed, in_features, nopairs)
    flat, gflat = x.reshape(-1, in_features), gy.reshape(-1, gy.shape[-1])
    gw = torch.zeros_like(w)
    gw[:, cols] = gflat.T @ (flat[:, cols] * scale)
    return F.linear(x, w, b), gy @ w, gw, gflat.sum(dim=0)


def layer_step(x, w, b, gy, nopairs):
    xi, wi, bi = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    y = fewbit.functional.linear_crs(xi, wi, bi, nopairs)
    y.backward(gy)
    return y.detach(), xi.grad, wi.grad, bi.grad


def test_the_layer_is_the_torch_formulation_with_the_columns_of_its_seed(lref):
    """fp32, the shapes of tests/golden/linear_ref.npz (and the same data as a 3-D batch): weight.grad against G^T (x[:, cols] * scale)
    scattered by torch, rtol 2e-4 of the largest entry (two fp32 GEMMs in another summation order: the tolerance of check_injected_draws);
    y, gx and gb are F.linear's"""
    x, w, b, gy = (lref[k].to(DEV) for k in ('lin_x', 'lin_w', 'lin_b', 'lin_gy'))
    nopairs = int(lref['crs_nopairs'])
    shapes = [(x, gy)]
    if x.dim() == 2 and x.shape[0] % 2 == 0:
        shapes.append((x.reshape(2, -1, x.shape[-1]), gy.reshape(2, -1, gy.shape[-1])))
    for s, (xs, gs) in enumerate(shapes):
        for nop in (nopairs, 1, 4 * w.shape[1]):
            torch.manual_seed(100 + s)
            seed = linear._draw_seed(None)
            torch.manual_seed(100 + s)
            y, gx, gw, gb = layer_step(xs, w, b, gs, nop)
            wy, wgx, wgw, wgb = torch_formulation(xs, w, b, gs, seed, nop)
            assert float((gw - wgw).abs().max()) <= 2e-4 * float(wgw.abs().max()), (s, nop)
            assert torch.count_nonzero(gw) > 0
            assert torch.equal(y, wy) and torch.equal(gx, wgx) and torch.equal(gb, wgb)


@pytest.mark.parametrize('dtype', DTYPES)
def test_manual_seed_reproduces_the_weight_gradient(dtype):
    x, w, b, gy = (torch.randn(s, device=DEV).to(dtype) for s in ((256, 96), (40, 96), (40, ), (256, 40)))
    grads = []
    for seed in (3, 3, 4):
        torch.manual_seed(seed)
        grads.append(layer_step(x, w, b, gy, 48)[2])
    assert torch.equal(bits(grads[0]), bits(grads[1])) and not torch.equal(grads[0], grads[2])


def sync_debug(step):
    """run `step` with torch.cuda.set_sync_debug_mode('error'); -> the error it raised, or None"""
    if not hasattr(torch.cuda, 'set_sync_debug_mode'):
        pytest.skip('this torch build has no torch.cuda.set_sync_debug_mode')
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        step()
        return None
    except RuntimeError as e:
        return e
    finally:
        torch.cuda.set_sync_debug_mode(prev)


def test_the_native_path_does_not_synchronise_and_the_fallbacks_do():
    """forward and backward under sync-debug mode 'error': nothing on the kernels; the PyTorch formulation (use_native_sketch(False), and a
    float64 tensor whatever the switch says) reads the number of hit columns back and raises -- which also shows which path ran"""
    x, w, b, gy = (torch.randn(s, device=DEV) for s in ((512, 128), (64, 128), (64, ), (512, 64)))
    layer_step(x, w, b, gy, 64)                                                         # (warm-up: libraries, the replay counter)
    torch.cuda.synchronize()
    for dtype in DTYPES:
        args = [t.to(dtype) for t in (x, w, b, gy)]
        layer_step(*args, 64)
        torch.cuda.synchronize()
        assert sync_debug(lambda: layer_step(*args, 64)) is None, dtype
    torch.cuda.synchronize()
    err = sync_debug(lambda: layer_step(*(t.double() for t in (x, w, b, gy)), 64))
    assert err is not None and 'synchroniz' in str(err)
    linear.use_native_sketch(False)
    err = sync_debug(lambda: layer_step(x, w, b, gy, 64))
    assert err is not None and 'synchroniz' in str(err)


def test_the_fallbacks_do_not_call_the_kernels(monkeypatch):
    """use_native_sketch(False) and float64 keep the PyTorch formulation: with the bindings replaced by ones that raise, they still run"""
    def refuse(*a, **k):
        raise AssertionError('the crs kernels were called')
    x, w, b, gy = (torch.randn(s, device=DEV) for s in ((64, 32), (8, 32), (8, ), (64, 8)))
    monkeypatch.setattr(cabi_x, 'crs_gather', refuse)
    monkeypatch.setattr(cabi_x, 'crs_scatter', refuse)
    with pytest.raises(AssertionError, match='crs kernels'):
        layer_step(x, w, b, gy, 16)
    gw = layer_step(*(t.double() for t in (x, w, b, gy)), 16)[2]
    assert gw.dtype == torch.float64 and torch.count_nonzero(gw) > 0
    linear.use_native_sketch(False)
    gw = layer_step(x, w, b, gy, 16)[2]
    assert torch.count_nonzero(gw) > 0 and int((gw != 0).any(dim=0).sum()) <= 16


def test_the_layer_is_captured_into_a_hipgraph_and_draws_fresh_columns_on_every_replay():
    """LinearCRS(768, 3072) bf16 on 4096 rows: forward + backward captured on one stream after one eager warm-up; three replays give three
    different weight gradients, each zero outside at most nopairs columns, and the mean over 64 replays is the exact gradient within the
    0.15 of tests/test_gpu_linear.py's statistics test.  (The PyTorch formulation cannot be captured: nonzero synchronises.)"""
    torch.manual_seed(7)
    lin = fewbit.LinearCRS(768, 3072, device=DEV, dtype=torch.bfloat16)
    nopairs = lin.nopairs
    x = torch.randn(4096, 768, device=DEV).to(torch.bfloat16)
    gy = torch.randn(4096, 3072, device=DEV).to(torch.bfloat16)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.autograd.grad(lin(x), lin.weight, gy)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gw, = torch.autograd.grad(lin(x), lin.weight, gy)
    exact = gy.float().T @ x.float()
    seen, acc = [], torch.zeros_like(exact)
    for r in range(64):
        g.replay()
        torch.cuda.synchronize()
        assert torch.isfinite(gw).all()
        if r < 3:
            seen.append(gw.clone())
            hit = int((gw != 0).any(dim=0).sum())
            assert 0 < hit <= min(nopairs, 768), hit
        acc += gw.float()
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2]) and not torch.equal(seen[0], seen[2])
    assert float(torch.linalg.norm(acc / 64 - exact) / torch.linalg.norm(exact)) <= 0.15
