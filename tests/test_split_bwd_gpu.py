"""The backward's split-operand GEMMs term by term.  The output gradient's columns are disjoint across molecules
and the weights are the signed-permutation probes, so a column stays with one molecule all the way down and every
element of every weight gradient sums about a dozen products of full-mantissa operands, at any batch size
(split_cases.py, "the backward").  Each stage of wdmpnn_backward -- the readout adjoint, dA = dZo W_o[:, Fa:], the
transposed gathers, the scale words (to the byte), dZ_{t-1} = act'(Z_{t-1}) (Y_t W_h) + residual, the weight
gradients and the bias sums -- is held to its elementwise bound against a float64 reference built from the buffer
the stage itself read: 2^-21 sum |a| |b| for the GEMMs, plus the fp16-pair floor where pairs multiply.  Elements
whose bound is 0 must be exactly 0: most of every gradient, so a stray row or column shows.

test_split_bwd_ref.py shows on these same inputs that the complete schemes stay under every bound and that a GEMM
that lost one plane product puts a quarter or more of its elements over.

The tests call wdmpnn_backward themselves, as mpn._backward_call does, on a NaN-filled scratch they keep and into
NaN-filled gradients, and find the scratch buffers through wdmpnn_debug_bwd_offsets."""
import ctypes

import numpy as np
import pytest
import torch

import split_cases as sc
from chemprop_amd import _native
from chemprop_amd.featurization import get_atom_fdim, get_bond_fdim
from chemprop_amd.mpn import MPNEncoder

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
FA = get_atom_fdim()
GRADS = {'W_i': 'W_i.weight', 'b_i': 'W_i.bias', 'W_h': 'W_h.weight', 'b_h': 'W_h.bias', 'W_o': 'W_o.weight',
         'b_o': 'W_o.bias'}


def _nan_bytes(nbytes):
    return torch.full((-(-nbytes // 4),), float('nan'), dtype=torch.float32, device=DEV).view(torch.uint8)


def _run(name):
    """(inputs, saved forward, backward buffers and gradients, the debug export) of one case on the device."""
    inp = sc.bwd_inputs(name)
    g, plan, H, T = inp.g, inp.plan, inp.H, inp.T
    enc = MPNEncoder(inp.args, FA, get_bond_fdim(atom_messages=inp.atom))
    sc.load_parameters(enc, inp.params)
    enc = enc.to(DEV).train()
    out, (gs, cfg, pstruct, ws, ws_bytes, packed, dg) = enc._train_forward(g)
    assert not dg.built_on_device
    for k, c in zip(('msg_t', 'agg_t'), sc.bwd_gathers(g, inp.atom)[2:]):  # (the lists the references transpose)
        h = dg.host_csr[k]
        assert np.array_equal(h.ptr, c.ptr) and np.array_equal(h.idx, c.idx) and np.array_equal(h.coef, c.coef)

    L = _native.lib()
    a = (ctypes.byref(gs), ctypes.byref(pstruct), ctypes.byref(cfg))
    nbytes = ctypes.c_size_t()
    _native.check(L.wdmpnn_backward_workspace_bytes(*a, ctypes.byref(nbytes)), 'backward workspace')
    L.wdmpnn_debug_bwd_offsets.argtypes = [ctypes.c_void_p] * 4
    L.wdmpnn_debug_bwd_offsets.restype = ctypes.c_int
    offs = (ctypes.c_size_t * 21)()
    _native.check(L.wdmpnn_debug_bwd_offsets(ctypes.addressof(gs), ctypes.addressof(pstruct), ctypes.addressof(cfg),
                                             ctypes.addressof(offs)), 'backward offsets')
    off = dict(zip(('dZo', 'dA', 'dZ0', 'dZ1', 'dRes', 'dX', 'words', 'mwords', 'total', 'blocked', 'ro_fused', 'bm',
                    'o_kps', 'o_ns', 'h_kps', 'h_ns', 'i_kps', 'i_ns', 'A', 'X', 'ldx'), offs))
    assert off['total'] == nbytes.value
    # the path and the plans the references and the CPU emulation assume
    assert off['blocked'] == int(plan.blocked) and off['ro_fused'] == 1 and off['bm'] == plan.bm
    assert (off['o_kps'], off['o_ns']) == plan.o and (off['h_kps'], off['h_ns']) == plan.h
    assert (off['i_kps'], off['i_ns']) == plan.i and off['ldx'] == plan.ldx

    scratch = _nan_bytes(nbytes.value)
    grads = {k: torch.full_like(t, float('nan')) for k, t in
             ((k, dict(enc.named_parameters()).get(n)) for k, n in GRADS.items()) if t is not None}
    wg = _native.WdGrads()
    for k, t in grads.items():
        setattr(wg, k, t.data_ptr())
    dout = torch.from_numpy(inp.dout).to(DEV)
    _native.check(L.wdmpnn_backward(*a, ws.data_ptr(), ws_bytes, dout.data_ptr(), scratch.data_ptr(), nbytes.value,
                                    ctypes.byref(wg), _native.current_stream(DEV)), 'backward')
    torch.cuda.synchronize()
    sn, wn = scratch.cpu().numpy(), ws.cpu().numpy()

    def rows(buf, o, rows_p, ld, n, cols, clean=True):
        x = buf[o:o + rows_p * ld * 4].view(np.float32).reshape(rows_p, ld)
        if clean:  # everything written is finite, the padding rows and columns are zero
            assert np.isfinite(x).all()
            assert not x[n:].any() and not x[:, cols:].any()
        return x[:n, :cols].copy()

    lay = _native.WdSaved()
    _native.check(L.wdmpnn_saved_layout(*a, ctypes.byref(lay)), 'saved layout')
    assert (lay.depth, lay.rows, lay.atom_rows, lay.ld) == (T, plan.R, plan.Va, plan.Hk)
    fwd = sc.Bag(Z=[rows(wn, lay.z[t], plan.R, plan.Hk, plan.R, H, False) for t in range(T)],
                 Zo=rows(wn, lay.zo, plan.Va, plan.Hk, plan.Va, H, False),
                 A=rows(wn, off['A'], plan.Va, plan.Hk, plan.Va, H, False))
    if not plan.blocked:
        X = rows(wn, off['X'], plan.R, plan.ldx, plan.R, plan.ldx, False)
        fwd.X = X[:, :H]
        if inp.atom:
            fwd.Xf = X[:, plan.Hk:plan.Hk + inp.Fb]
    assert all(np.isfinite(x).all() for x in fwd.Z + [fwd.Zo, fwd.A])

    def bonds(key):
        return rows(sn, off[key], plan.Rp, plan.Hk, plan.R, H)

    b = sc.Bag({k: t.cpu().numpy() for k, t in grads.items()})
    b.b_i, b.b_h = b.get('b_i'), b.get('b_h')
    assert all(np.isfinite(x).all() for x in b.values() if x is not None)
    b.dZo = rows(sn, off['dZo'], plan.Vap, plan.Hk, plan.Va, H)
    b.dA = rows(sn, off['dA'], plan.Vap, plan.Hk, plan.Va, H)
    b.dRes = bonds('dRes')
    # (the two dZ buffers alternate: dZ_{T-1} in the first, each layer's dZ_{t-1} in the other)
    if T == 2:
        b.dZ_last, b.dZ0 = bonds('dZ0'), bonds('dZ1')
    else:
        b.dZ_last, b.dZ1, b.dZ0 = None, bonds('dZ1'), bonds('dZ0')
    b['Y' if plan.blocked else 'dX'] = bonds('dX')
    if plan.blocked:
        b.words = sn[off['words']:off['words'] + plan.Rp * plan.Hk // 256].view(np.uint32).copy()
        b.mwords = sn[off['mwords']:off['mwords'] + (plan.Rp // plan.bm) * (plan.Hk // 64) * 4].view(np.uint32).copy()
    return inp, fwd, b


@pytest.mark.parametrize('name', list(sc.BWD_CASES))
def test_backward_stage_by_stage(name):
    """Worst |error| / bound per stage on the MI355X (DESIGN.md section 2 holds the table)."""
    inp, fwd, b = _run(name)
    case = inp.case
    assert all((z[1:] > 0).mean() > 0.2 for z in fwd.Z)  # (the kinks leave the backward something to carry)
    if case['kind'] == 'hub':
        assert inp.g.molecule_blocks() is None
    if name == 'tiny-b96-h300':
        assert inp.plan.h[0] >= 64 and inp.plan.h[1] >= 2
    stages = sc.bwd_stages(inp, fwd, b)
    assert {s[0] for s in stages} >= {'dW_h', 'dW_i', 'dW_o[:, :Fa]', 'dW_o[:, Fa:]', 'db_o'}
    if case.get('bias'):
        assert {s[0] for s in stages} >= {'db_h', 'db_i'}
    if inp.atom:  # the bond-feature half of dW_h: its weights are zero, its gradient is not
        assert b.W_h[:, inp.H:].any() and not inp.params['W_h.weight'].numpy()[:, inp.H:].any()
    bad = []
    for stage, got, ref, bound in stages:
        assert np.isfinite(np.asarray(got, np.float64)).all(), (name, stage)
        top, n_over, _ = sc.stage_worst(got, ref, bound)
        live = float((np.asarray(bound) > 0).mean())
        print(f'\nbwd {name} {stage}: worst |error| / bound {top:.3f} ({n_over} over, {live:.3f} of the elements live)')
        if n_over:
            bad.append((stage, top, n_over))
        if stage not in ('words', 'mwords', 'dRes'):
            assert live > 0, (name, stage)
    assert not bad, (name, bad)
