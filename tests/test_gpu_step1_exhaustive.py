"""The 1-bit family (stepwise1_*_kernel) against definitions restated outside the oracle: tests/step1_reference.py, a plain fp32 torch-on-host
restatement that tests/test_step1_rules_host.py holds to ATen's own forward and autograd on every 16-bit input.

Per function, parameter set and dtype: value bits, packed state and gradient (gy = the inputs rotated by 12 345) of the kernels equal the
restatement's, for every 16-bit pattern (fp32: helpers.probe_patterns, which adds the +-1 / +-2 ulp neighbours of every kink 0, +-p0, p1, +-3, 6),
through the tile body and through the element-wise tail (helpers.run_body / run_tail), at one and at two groups per lane.  The parameter sets include
values the 16-bit dtypes cannot represent (0.3, 1/3, 0.01, 0.1): the kernels compare and compute with float32(p), and so does the restatement.
ATen's host result is a second reference where it is defined the same way: parameters the dtype represents, finite nonzero inputs."""
import pytest
import torch

import step1_reference as ref
from fewbit_amd import cabi
from helpers import GEOMETRIES, STEP1_CASES, STREAM_TUNE_KEYS, case_id, differing, kinks, probe_patterns, run_geometry, set_groups_per_lane

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = (torch.float32, torch.float16, torch.bfloat16)


@pytest.fixture(autouse=True)
def _restore_launch_policy():
    yield
    cabi.tune(**{k: -1 for k in STREAM_TUNE_KEYS})


def report(what, got, want, x, problems):
    d = differing(got, want)
    if bool(d.any()):
        idx = d.nonzero().flatten()[:4].tolist()
        problems.append(f'{what}: {int(d.sum())} inputs differ, first x = {x[idx].tolist()}: kernel {got[idx].tolist()}, restatement {want[idx].tolist()}')
        print(problems[-1])


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
@pytest.mark.parametrize('name,p', STEP1_CASES, ids=case_id)
def test_stepwise1_is_the_restated_definition(name, p, dtype):
    x = probe_patterns(dtype, kinks(p))
    gy = torch.roll(x, 12345)
    y_ref, bit_ref = ref.rules(name, x, *p)
    gx_ref = ref.backward(name, gy, bit_ref, *p[:1])
    codes_ref = bit_ref.to(torch.int32)

    def op(xs, gs):
        y, state = cabi.stepwise1_forward(name, xs, *p)
        return y, cabi.unpack_codes(state, xs.numel(), 1), cabi.stepwise1_backward(name, gs, state, *p[:1]), cabi.stepwise1_backward(name, torch.ones_like(gs), state, *p[:1])
    problems = []
    for where, u in GEOMETRIES:
        set_groups_per_lane(u)
        y, codes, gx, g1 = run_geometry(where, op, x, gy)
        report(f'{name}{p} {dtype} {where} U={u} value', y, y_ref, x, problems)
        report(f'{name}{p} {dtype} {where} U={u} state bit', codes, codes_ref, x, problems)
        report(f'{name}{p} {dtype} {where} U={u} gradient', gx, gx_ref, x, problems)
    assert not problems, '\n'.join(problems)

    # the packed bytes themselves (the layout, not only the unpacked codes), one tail call and its ragged last group
    xs = x[:507].to(DEV)
    _, state = cabi.stepwise1_forward(name, xs, *p)
    assert torch.equal(state.cpu(), ref.pack_bits(bit_ref[:507]))

    # ATen on the host, where it is the same function: the dtype holds the parameters, the input is finite and nonzero (g1: gy = 1, last geometry).
    # The sign of a ZERO result of softshrink is not compared: ATen's fp32 host kernel gives +0 in its vectorised part and a * 0 (-0 for a negative
    # input) in its scalar remainder, so there it depends on the element's position; the restatement above already pins the kernels to +0.
    if all(float(torch.tensor(q, dtype=torch.float32).to(dtype).float()) == float(torch.tensor(q, dtype=torch.float32)) for q in p):
        y_aten, g_aten = ref.aten(name, x, *p)
        plain = torch.isfinite(x) & (x != 0)
        dy = differing(y, y_aten) & plain
        if name == 'softshrink':
            dy &= ~((y == 0) & (y_aten == 0))
        assert not bool(dy.any()), (name, p, x[dy][:4], y[dy][:4], y_aten[dy][:4])
        dg = differing(g1, g_aten) & plain
        assert not bool(dg.any()), (name, p, x[dg][:4], g1[dg][:4], g_aten[dg][:4])
