"""The sampled transforms behind a random sign per row on the GPU.  The yardstick is exact: negation is exact in fp32, fp16 and bf16, so
``sampled_d{c,f}t_signed(m, rows, p, seed)`` has to equal, bit for bit, ``sampled_d{c,f}t_zext_seeded`` of ``m`` with the rows of
``sampled_signs(seed, valid_rows)`` negated.  Then the seed as a device word (and a recorded launch that reads it), the refusals, and the layer
with ``use_sign_flips(True)``."""
import pytest
import torch
import torch.nn.functional as F

import fewbit_amd as fewbit
from fewbit_amd import cabi_x, linear

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
# (rows, valid_rows, features, ld - features, p).  Every row family (2^k, 3, 5, 9, 7, 15 x 2^k; 32768 = 256 x 128: the pass A tile above 64 KiB)
# with a ragged valid_rows and an edge feature tile (1, 65 = 64 + 1, 136 = 2 x 64 + 8); valid_rows in {rows, rows - 1, rows / 2 + 1, 1};
# features in {1, 64, 65, 136}; ld in {features, features + 8}; p in {1, 37, rows}.
CASES = ((256, 256, 64, 0, 37), (256, 255, 65, 8, 256), (256, 129, 1, 0, 1), (256, 1, 136, 8, 37),
         (768, 385, 65, 0, 37), (768, 768, 136, 8, 1),
         (1280, 1279, 65, 8, 37), (1280, 1, 64, 0, 1280),
         (2304, 1153, 136, 0, 37),
         (3584, 3583, 1, 8, 37), (3584, 1793, 65, 0, 1),
         (3840, 1921, 65, 8, 37),
         (32768, 32767, 65, 0, 37), (32768, 32768, 64, 8, 37))


@pytest.fixture(autouse=True)
def _native():
    prev = linear.use_native_sketch(True)
    yield
    linear.use_native_sketch(prev)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _data(valid, features, ld, dtype, seed):
    """-> (the valid x ld buffer, finite values with some exact zeros; its valid x features view)"""
    g = torch.Generator().manual_seed(seed)
    base = (torch.randint(-64, 65, (valid, ld), generator=g).float() / 16).to(dtype).to(DEV)
    return base, base[:, :features]


def _negated(base, features, seed):
    """the buffer with the rows of sampled_signs(seed, rows of it) negated, as the view the kernels take (zeros become -0: a sign bit)"""
    flip = cabi_x.sampled_signs(seed, base.shape[0]).to(DEV)
    return torch.where(flip[:, None], -base, base)[:, :features]


def _signed(kind, x, rows, p, seed, scale, out_dtype=None, **kw):
    if kind == 'dct':
        return cabi_x.sampled_dct_signed(x, rows, p, seed, scale, **kw)
    return cabi_x.sampled_dft_signed(x, rows, p, seed, scale, out_dtype, **kw)


def _unsigned(kind, x, rows, p, seed, scale, out_dtype=None):
    if kind == 'dct':
        return cabi_x.sampled_dct_zext_seeded(x, rows, p, seed, scale)
    return cabi_x.sampled_dft_zext_seeded(x, rows, p, seed, scale, out_dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', ('dct', 'dft'))
def test_the_signed_call_equals_the_unsigned_call_on_the_negated_rows_bit_for_bit(kind, dtype):
    for n, (rows, valid, features, pad, p) in enumerate(CASES):
        seed = 0x51ed270b0000 + 977 * n
        base, x = _data(valid, features, features + pad, dtype, 31 * n + features)
        flipped = cabi_x.sampled_signs(seed, valid)
        assert valid == 1 or 0 < int(flipped.sum()) < valid
        xn = _negated(base, features, seed)
        assert xn.stride(0) == x.stride(0) == features + pad
        for out_dtype in ((None, ) if kind == 'dct' else (torch.float32, dtype)):
            got = _signed(kind, x, rows, p, seed, 1.5, out_dtype)
            want = _unsigned(kind, xn, rows, p, seed, 1.5, out_dtype)
            assert got.shape == want.shape and got.dtype == want.dtype
            assert torch.equal(_bits(got), _bits(want)), (kind, dtype, out_dtype, rows, valid, features, pad, p)
            if bool(flipped.any()) and valid > 1:                       # (and the signs are not a no-op)
                assert not torch.equal(_bits(got), _bits(_unsigned(kind, x, rows, p, seed, 1.5, out_dtype)))


@pytest.mark.parametrize('kind', ('dct', 'dft'))
def test_the_seed_as_a_device_word_gives_the_bits_of_the_seed_by_value_and_a_recorded_launch_reads_it_anew(kind):
    rows, valid, features, p, dtype = 768, 700, 65, 37, torch.bfloat16
    _, x = _data(valid, features, features + 8, dtype, 5)
    s1, s2 = 0x1234567890abcdef, 0x0fedcba987654321
    by_value = [_signed(kind, x, rows, p, s, 1.0) for s in (s1, s2)]
    assert not torch.equal(_bits(by_value[0]), _bits(by_value[1]))
    # reproducible: the same arguments give the same bits
    assert torch.equal(_bits(_signed(kind, x, rows, p, s1, 1.0)), _bits(by_value[0]))
    word = torch.tensor([s1], dtype=torch.int64, device=DEV)
    assert torch.equal(_bits(_signed(kind, x, rows, p, word, 1.0)), _bits(by_value[0]))
    out = torch.empty_like(by_value[0])
    workspace = torch.empty(cabi_x.sampled_dft_workspace_bytes(rows, features, p, dtype), dtype=torch.uint8, device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _signed(kind, x, rows, p, word, 1.0, out=out, workspace=workspace)
    for s, want in ((s1, by_value[0]), (s2, by_value[1]), (s1, by_value[0])):
        word.fill_(s)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(want)), hex(s)


def test_refused_calls_launch_nothing_and_leave_the_output_alone():
    L = cabi_x.lib()
    err = L.fewbit_hipx_last_error
    rows, features, p = 768, 8, 4
    x = torch.ones(rows, features, device=DEV)
    out = torch.full((2, p, features), 7.0, device=DEV)
    need = cabi_x.sampled_dft_workspace_bytes(rows, features, p, torch.float32)
    ws = torch.zeros(need + 64, dtype=torch.uint8, device=DEV)
    word = torch.zeros(2, dtype=torch.int64, device=DEV)
    xp, op, wp = x.data_ptr(), out.data_ptr(), ws.data_ptr()
    dct = lambda *a: L.fewbit_hipx_sampled_dct_signed(*a)
    dft = lambda *a: L.fewbit_hipx_sampled_dft_signed(*a)
    torch.cuda.synchronize()
    for call, name in ((lambda **k: dct(k.get('dt', 0), k.get('x', xp), k.get('rows', rows), k.get('valid', rows), features, k.get('ld', features), 1, k.get('word'), p, 1.0,
                                        op, k.get('ws', wp), k.get('wb', need), None), b'sampled_dct_signed'),
                       (lambda **k: dft(k.get('dt', 0), k.get('x', xp), k.get('rows', rows), k.get('valid', rows), features, k.get('ld', features), 1, k.get('word'), p, 1.0,
                                        k.get('odt', 0), op, k.get('ws', wp), k.get('wb', need), None), b'sampled_dft_signed')):
        assert call(rows=700) == -2 and b'rows = 700' in err() and name in err()
        assert call(valid=0) == -1 and b'valid_rows' in err() and name in err()
        assert call(valid=rows + 1) == -1 and b'valid_rows' in err()
        assert call(dt=9) == -1 and b'dtype' in err()
        assert call(wb=need - 1) == -1 and b'workspace' in err()
        assert call(ws=wp + 8) == -1 and b'aligned' in err()
        assert call(x=None) == -1 and b'null' in err()
        assert call(ld=features - 1) == -1 and b'leading dimension' in err()
        assert call(word=word.data_ptr() + 4) == -1 and b'8-byte aligned' in err() and name in err()
        assert call(ld=1 << 23) == -2 and b'4 GiB' in err()
    assert dft(2, xp, rows, rows, features, features, 1, None, p, 1.0, 1, op, wp, need, None) == -1 and b'out_dtype' in err()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and not bool(ws.any())
    with pytest.raises(fewbit.cabi.FewbitHipError, match='sampled_dct_signed'):
        cabi_x.sampled_dct_signed(x[:700], 700, p, 1)


def _host_seed(k):
    """the seed the layer draws from a host generator seeded with k (linear._draw_seed: one randint of the generator)"""
    return int(torch.randint(0, 2**62, (), dtype=torch.int64, generator=torch.Generator().manual_seed(k)).item())


@pytest.mark.parametrize('dtype', (torch.bfloat16, torch.float32))
@pytest.mark.parametrize('kind', ('dct', 'dft'))
@pytest.mark.parametrize('rows', (256, 200))
def test_the_layer_with_signs_is_the_layer_without_on_negated_rows_bit_for_bit(kind, dtype, rows):
    """256 rows (a row count with a kernel) and 200 rows with use_row_extension(True) (zero-extended to 256): grad_weight of the switch-on
    layer equals, bit for bit, the switch-off layer's on the row-negated input and grad_output under the same seed; forward is F.linear;
    grad_input and grad_bias are exact; the node saves what the unsigned node saves."""
    features, outs, p, k = 70, 12, 64, 17 + rows
    g = torch.Generator().manual_seed(rows)
    x = (1 + torch.randn(rows, features, generator=g)).to(dtype).to(DEV)
    w = (torch.randn(outs, features, generator=g) * 0.3).to(dtype).to(DEV)
    b = torch.randn(outs, generator=g).to(dtype).to(DEV)
    gy = torch.randn(rows, outs, generator=g).to(dtype).to(DEV)
    flip = cabi_x.sampled_signs(_host_seed(k), rows).to(DEV)[:, None]
    assert 0 < int(flip.sum()) < rows

    def step(xv, gv):
        xi, wi, bi = xv.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
        y = fewbit.functional.linear_grp(xi, wi, bi, proj_dim=p, matmul=kind, generator=torch.Generator().manual_seed(k))
        saved = [(tuple(t.shape), t.dtype) for t in y.grad_fn.saved_tensors]
        y.backward(gv)
        return y.detach(), xi.grad, bi.grad, wi.grad, saved

    prev_ext, prev_flip = linear.use_row_extension(rows == 200), linear.use_sign_flips(True)
    try:
        path = linear.sampled_transform_path(kind, x)
        assert f'fewbit_hipx_sampled_{kind}_signed' in path and ('zero-extended to 256 rows' in path) == (rows == 200)
        y, gx, gb, gw, saved = step(x, gy)
        linear.use_sign_flips(False)
        assert 'signed' not in linear.sampled_transform_path(kind, x)
        _, _, _, gw_off, saved_off = step(torch.where(flip, -x, x), torch.where(flip, -gy, gy))
        _, _, _, gw_plain, _ = step(x, gy)
    finally:
        linear.use_row_extension(prev_ext)
        linear.use_sign_flips(prev_flip)
    assert torch.equal(y, F.linear(x, w, b)) and torch.equal(gx, gy @ w) and torch.equal(gb, gy.sum(0))
    assert torch.equal(_bits(gw), _bits(gw_off)) and not torch.equal(_bits(gw), _bits(gw_plain))
    assert saved == saved_off and len(saved) == (3 if kind == 'dft' else 2)
    assert saved[0] == ((p, features), dtype)


@pytest.mark.parametrize('kind', ('dct', 'dft'))
def test_backward_on_the_gpu_follows_what_the_forward_did(kind):
    rows, features, outs, p, k = 256, 64, 8, 64, 5
    x = torch.randn(rows, features, device=DEV)
    gy = torch.randn(rows, outs, device=DEV)
    grads = {}
    for forward_on, backward_on in ((True, True), (True, False), (False, False), (False, True)):
        w = torch.ones(outs, features, device=DEV, requires_grad=True)
        prev = linear.use_sign_flips(forward_on)
        try:
            y = fewbit.functional.linear_grp(x, w, None, proj_dim=p, matmul=kind, generator=torch.Generator().manual_seed(k))
            linear.use_sign_flips(backward_on)
            y.backward(gy)
        finally:
            linear.use_sign_flips(prev)
        grads[forward_on, backward_on] = w.grad
    assert torch.equal(grads[True, True], grads[True, False]) and torch.equal(grads[False, False], grads[False, True])
    assert not torch.equal(grads[True, True], grads[False, False])


@pytest.mark.parametrize('kind', ('dct', 'dft'))
def test_a_captured_step_with_signs_draws_afresh_on_every_replay(kind):
    """capture into torch.cuda.graph after one eager call works, and two replays give different weight gradients"""
    rows, features, outs, p, dtype = 256, 64, 16, 64, torch.bfloat16
    prev = linear.use_sign_flips(True)
    try:
        lin = fewbit.RandomizedLinear(features, outs, proj_dim=p, matmul=kind, bias=False, device=DEV, dtype=dtype)
        x = torch.randn(rows, features, device=DEV, dtype=dtype, requires_grad=True)
        wgt = torch.randn(rows, outs, device=DEV, dtype=dtype)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            torch.autograd.grad((lin(x) * wgt).sum(), lin.weight)                  # the one eager call
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            gw, = torch.autograd.grad((lin(x) * wgt).sum(), lin.weight)
        seen = []
        for _ in range(2):
            g.replay()
            torch.cuda.synchronize()
            assert bool(torch.isfinite(gw.float()).all())
            seen.append(gw.clone())
        assert not torch.equal(seen[0], seen[1])
    finally:
        linear.use_sign_flips(prev)
