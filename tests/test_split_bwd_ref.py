"""What makes test_split_bwd_gpu.py meaningful, shown on its own inputs by CPU emulation (oracle/split_ref.py):
with every plane product present no element of any backward stage is over its bound (split_cases.bwd_stages),
and with any one product removed from one of the backward's GEMMs a quarter or more of that GEMM's elements whose
bound is not zero are over it -- the thresholds of test_split_ref.py.

The forward is emulated with the complete bf16x3 scheme, the backward chain runs in numpy, its GEMMs through
``split_ref.mm_x6`` / ``mm_h2``: the weight gradients with transposed operands, split and chunked as the kernel's
plan splits them, the pair forms with the scales of the words the emulated chain itself publishes."""
import functools

import pytest

import split_cases as sc
from oracle import split_ref as sr

X6_DROPS = ('hm', 'mh', 'hl', 'lh', 'mm')
H2_DROPS = ('hl', 'lh')


@functools.lru_cache(maxsize=None)
def _complete(name):
    inp = sc.bwd_inputs(name)
    fwd = sc.emulate_forward(inp)
    return inp, fwd, sc.emulate_backward(inp, fwd)


@pytest.mark.parametrize('name', list(sc.BWD_CASES))
def test_case_takes_the_shapes_it_is_meant_for(name):
    inp, fwd, _ = _complete(name)
    case, plan = inp.case, inp.plan
    assert (inp.g.molecule_blocks() is not None) == (case['kind'] != 'hub')
    if name == 'tiny-b96-h300':  # split and chunk boundaries inside the reduction, molecules straddling them
        kps, nsplit = plan.h
        assert kps >= 64 and nsplit >= 2
        assert any(b0 // kps != (b0 + n - 1) // kps for b0, n in inp.g.b_scope if n)
    if case['kind'] == 'hub':
        assert max(n for _, n in inp.g.b_scope) > sc.OWNER_MAX_BONDS
        hub = max(range(len(inp.g.b_scope)), key=lambda i: inp.g.b_scope[i][1])
        assert hub not in inp.owner and not inp.dout[hub].any()
    # every molecule that owns columns owns at least one, the features and dout have full mantissas
    h, m, l = sr.split3(inp.f_in[1:])
    assert (m != 0).mean() > 0.9 and (l != 0).mean() > 0.9
    assert all((z[1:] > 0).mean() > 0.2 for z in fwd.Z)


@pytest.mark.parametrize('name', list(sc.BWD_CASES))
def test_complete_schemes_stay_under_every_bound(name):
    inp, fwd, b = _complete(name)
    for stage, got, ref, bound in sc.bwd_stages(inp, fwd, b):
        top, n_over, _ = sc.stage_worst(got, ref, bound)
        print(f'{name} {stage} complete: worst ratio {top:.3f}, live {float((bound > 0).mean()):.3f}')
        assert n_over == 0 and top <= 1.0, (name, stage, top, n_over)


def _drops():
    for name, case in sc.BWD_CASES.items():
        shape = sc.Bag(plan=sc.Bag(blocked=case['path'] == 'blocked'), T=case['depth'], atom=bool(case.get('atom')))
        for gemm, (scheme, stages) in sc.bwd_gemms(shape).items():
            if not case.get('only') or any(s.startswith(case['only']) for s in stages):  # (the stages the case checks)
                yield name, gemm, scheme


@pytest.mark.parametrize('name,gemm,scheme', list(_drops()))
def test_one_lost_product_puts_a_quarter_over(name, gemm, scheme):
    inp, fwd, base = _complete(name)
    stages = sc.bwd_gemms(inp)[gemm][1]
    if inp.only:
        stages = tuple(s for s in stages if s.startswith(inp.only))
    for drop in (X6_DROPS if scheme == 'x6' else H2_DROPS):
        b = sc.emulate_backward(inp, fwd, (gemm, drop), base)
        seen = 0
        for stage, got, ref, bound in sc.bwd_stages(inp, fwd, b):
            if stage not in stages:
                continue
            seen += 1
            top, _, share = sc.stage_worst(got, ref, bound)
            print(f'{name} {stage} without {drop}: worst ratio {top:.1f}, over the bound {share:.2f}')
            assert share >= 0.25, (name, stage, drop, share)
        assert seen == len(stages)
