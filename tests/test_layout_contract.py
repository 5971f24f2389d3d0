"""CPU: the sizes and offsets the library derives from (graph, parameters, configuration) -- packed
weights, forward and backward workspaces, the saved pre-activations and the fused forward's intermediate
buffers -- equal tests/golden/layout_contract.json, recorded by tools/make_layout_golden.py from the
library before the forward path's decisions moved into Dims.  Host-only like test_native_abi._structs:
device_graph('cpu', ...), pointers are offsets, nothing is launched."""
import ctypes
import json
import os

import numpy as np
import pytest

from chemprop_amd import _native
from chemprop_amd import synthetic
from chemprop_amd.featurization import BatchMolGraph

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'layout_contract.json')
BATCHES = (('polymer', 4), ('qm9', 2))
HIDDEN = (64, 300, 320, 512)
DEPTH = (2, 3, 5)
VARIANTS = (_native.VARIANT_DEFAULT, _native.VARIANT_F32, _native.VARIANT_FOUR_LAUNCH, _native.VARIANT_STAGED,
            _native.VARIANT_PAIRS, _native.variant_debug(_native.DEBUG_PAIRS, 3),
            _native.variant_debug(_native.DEBUG_STAGED, 3))
assert VARIANTS == (0, 9, 11, 12, 13, 113, 123)
# the optional arrays a CPU device graph leaves null; set to non-zero offsets, the blocked (planes) and with
# the code arrays the embed, pair and one-launch paths are reached
PLANES = ('f_atoms_x6', 'f_bonds_x6', 'blocks', 'bond_blk_row', 'f_atoms_blk_x6', 'msg_ell_idx', 'msg_ell_coef',
          'atom_ell_idx', 'atom_ell_coef')
CODES = ('atom_codes', 'bond_src_blk', 'bond_tail')
GROUPS = [(kind, n, msg) for kind, n in BATCHES for msg in ('bond', 'atom')]


def cases(kind, n, msg):
    """(key, arrays, hidden, depth, save, bias, variant, extra) of one batch and message mode.  Every value of
    every axis around the base point (hidden 300, depth 3, inference, no bias), crossed where the forward
    path's choice depends on the pair: hidden x variant (pair tiles need 80 | Hk, the one-launch forward Hk
    320), depth x variant, save x variant, save x bias (atom messages block without biases only).  The
    graphs without the code arrays (polymer only) take the two GEMM families and the staged layers; one
    descriptor case, its refusal without W_d, and undirected (bond messages run, atom messages are refused)."""
    pts = []
    for arrays in ('codes',) + (('planes', 'plain') if kind == 'polymer' else ()):
        variants = (0, 9, 12) if arrays != 'codes' else VARIANTS if msg == 'bond' else (0, 9, 12, 113)
        pts += [(arrays, h, 3, 0, 0, v) for h in HIDDEN for v in variants]
        pts += [(arrays, 300, t, 0, 0, v) for t in DEPTH for v in variants]
        pts += [(arrays, 300, 3, 1, 0, v) for v in variants]
        pts += [(arrays, 300, 3, s, 1, 0) for s in (0, 1)]
    out = [(f'{kind}{n}|{msg}|{a}|h{h}|d{t}|s{s}|b{b}|v{v}', a, h, t, s, b, v, '') for a, h, t, s, b, v in dict.fromkeys(pts)]
    if kind == 'polymer':
        for extra in ('desc', 'desc_no_Wd', 'undirected'):
            out.append((f'{kind}{n}|{msg}|codes|h300|d3|s0|b0|v0|{extra}', 'codes', 300, 3, 0, 0, 0, extra))
    return out


_GRAPHS = {}


def graph_struct(kind, n, msg, arrays):
    if (kind, n, msg) not in _GRAPHS:
        g = BatchMolGraph(synthetic.make_batch(kind, n, 0))
        _GRAPHS[kind, n, msg] = g.device_graph('cpu', msg == 'atom').struct, np.asarray(g.molecule_blocks())
    base, blocks = _GRAPHS[kind, n, msg]
    s = _native.WdGraph.from_buffer_copy(base)
    names = {'plain': (), 'planes': PLANES, 'codes': PLANES + CODES}[arrays]
    for i, f in enumerate(names):
        if not getattr(s, f):
            setattr(s, f, 4096 * (i + 1))
    if names:
        s.n_blocks = len(blocks)
        s.blk_max_bonds, s.blk_max_atoms = int(blocks[:, 1].max()), int(blocks[:, 3].max())
    return s


def query(L, kind, n, msg, case):
    """What the library answers for one case: {'rc': code} when it refuses the combination, else the sizes."""
    _, arrays, hidden, depth, save, bias, variant, extra = case
    s = graph_struct(kind, n, msg, arrays)
    p = _native.WdParams()
    p.hidden = hidden
    for f in ('W_i', 'W_h', 'W_o', 'b_o', 'zero_vec') + (('b_i', 'b_h') if bias else ()):
        setattr(p, f, 4096)
    if not save:  # inference runs on a cached pack, a training forward packs into its workspace
        p.packed, p.packed_bytes = 4096, 1 << 40
    if extra.startswith('desc'):
        s.atom_desc, s.desc_dim = 8192, 8
        if extra == 'desc':
            p.W_d = p.b_d = 4096
    c = _native.WdConfig()
    c.depth, c.activation, c.aggregation, c.aggregation_norm = depth, _native.ACTIVATIONS['ReLU'], 0, 100.0
    c.undirected, c.save_for_backward, c.gemm_variant = int(extra == 'undirected'), save, variant
    a = (ctypes.byref(s), ctypes.byref(p), ctypes.byref(c))
    nb = ctypes.c_size_t()
    rc = L.wdmpnn_packed_params_bytes(*a, ctypes.byref(nb))
    if rc:
        return {'rc': rc}
    res = {'pack': nb.value}
    assert L.wdmpnn_workspace_bytes(*a, ctypes.byref(nb)) == 0
    res['ws'] = nb.value
    if save:
        assert L.wdmpnn_backward_workspace_bytes(*a, ctypes.byref(nb)) == 0
        res['bwd'] = nb.value
        sv = _native.WdSaved()
        assert L.wdmpnn_saved_layout(*a, ctypes.byref(sv)) == 0
        res['saved'] = [sv.depth, sv.rows, sv.atom_rows, sv.ld, sv.zo] + list(sv.z[:depth])
    offs = (ctypes.c_size_t * 15)()
    L.wdmpnn_debug_fwd_offsets.argtypes = [ctypes.c_void_p] * 4
    L.wdmpnn_debug_fwd_offsets.restype = ctypes.c_int
    assert L.wdmpnn_debug_fwd_offsets(*(ctypes.addressof(x) for x in (s, p, c)), ctypes.addressof(offs)) == 0
    res['fwd'] = list(offs)
    return res


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize('kind,n,msg', GROUPS)
def test_layouts_equal_the_recorded_ones(golden, kind, n, msg):
    L = _native.lib()
    table = cases(kind, n, msg)
    got = {case[0]: query(L, kind, n, msg, case) for case in table}
    want = {k: golden[k] for k in got}  # (a missing key: the table and the golden file disagree)
    bad = [k for k in got if got[k] != want[k]]
    assert not bad, (len(bad), bad[0], got[bad[0]], want[bad[0]])


def test_table_reaches_both_layer_forms_and_the_refusals(golden):
    """The recorded table is not vacuous: D.pairs (word 9 of the fused forward's offsets) is 1 somewhere and 0
    somewhere, pair tiles are packed (word 10, W_o's) for some cases only, and refusals keep their codes."""
    assert len(golden) == sum(len(cases(*g)) for g in GROUPS)
    pairs = {v['fwd'][9] for v in golden.values() if 'fwd' in v}
    assert pairs == {0, 1}
    assert {bool(v['fwd'][10]) for v in golden.values() if 'fwd' in v} == {False, True}
    assert golden['polymer4|bond|codes|h300|d3|s0|b0|v0']['fwd'][9] == 1
    assert golden['polymer4|bond|codes|h300|d3|s0|b0|v12']['fwd'][9] == 0
    assert golden['polymer4|bond|codes|h300|d3|s0|b0|v123']['fwd'][9] == 1  # (debug: the tiles stay laid out)
    assert golden['polymer4|atom|codes|h300|d3|s0|b0|v0|undirected'] == {'rc': _native.ERR_UNSUPPORTED}
    assert golden['polymer4|bond|codes|h300|d3|s0|b0|v0|desc_no_Wd'] == {'rc': -1000}
    assert 'rc' not in golden['polymer4|bond|codes|h300|d3|s0|b0|v0|undirected']
