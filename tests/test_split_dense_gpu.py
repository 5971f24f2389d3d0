"""Dense accuracy at the contract: the split-operand GEMMs promise the error of an fp32 GEMM, so the HIP
training path (output and every parameter gradient, on dense inputs) is held to a small multiple of what the
fp32 oracle itself loses against float64, not to the 1e-5 parity bar.  The backward's weight-gradient GEMMs
are held term by term as well: an output gradient whose columns are disjoint across molecules makes their
sums a dozen products long (test_split_bwd_gpu.py).

e_hip: the HIP result against the float64 oracle, normwise per tensor (max |x - ref| / max |ref|), the float64
evaluation taking its kink decisions from the HIP forward's saved pre-activations (test_gpu_parity's recipe);
for the output also per row against the row's own maximum (the worst row).  e32: the fp32 oracle against the
same float64 evaluation with the same decisions.  Asserted: e_hip <= FACTOR * max(e32 of that tensor, e32 of
the case's output).  FACTOR 4: emulated on the CPU (tools/split_precision_sim.py) the complete schemes stay
within 1.5 x fp32 on these cases and the mildest scheme that lost a product sits near 10 x.  DESIGN.md §2
records the measured values."""
import numpy as np
import pytest
import torch

import golden_io
from chemprop_amd import TrainArgs, mpn, synthetic
from chemprop_amd.featurization import BatchMolGraph, get_atom_fdim, get_bond_fdim
from chemprop_amd.mpn import MPNEncoder
from oracle import mpn_ref

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
FACTOR = 4.0
CASES = {
    'polymer-b8-h64-d3': ('polymer', 8, 64, 3, {}),
    'polymer-b8-h300-d3-tanh-bias': ('polymer', 8, 300, 3, dict(activation='tanh', bias=True)),
    'qm9-b16-h96-d4-elu': ('qm9', 16, 96, 4, dict(activation='ELU')),
}


def _rows(x, ref):
    """The worst row of the output, each row against its own maximum."""
    return float((np.abs(x - ref).max(axis=1) / np.abs(ref).max(axis=1)).max())


def _reference(cpu, trainable, graph, args, R, dtype, kinks):
    p = {n: t.detach().clone().to(dtype).requires_grad_(n in trainable) for n, t in cpu.items()}
    out = mpn_ref.encoder_forward(p, graph, args, dtype=None if dtype == torch.float32 else dtype, masks=kinks)
    (out * R.to(dtype)).sum().backward()
    res = {'output': out.detach().numpy()}
    res.update({n: t.grad.numpy() for n, t in p.items() if t.grad is not None})
    return res


@pytest.mark.parametrize('name', list(CASES))
def test_hip_error_is_a_small_multiple_of_fp32s(name):
    kind, b, hidden, depth, extra = CASES[name]
    args = TrainArgs(hidden_size=hidden, depth=depth, **extra)
    graph = BatchMolGraph(synthetic.make_batch(kind, b, 100 + b))
    enc = MPNEncoder(args, get_atom_fdim(), get_bond_fdim())
    synthetic.fill_parameters(enc, b)
    cpu = {n: t.detach().clone() for n, t in enc.named_parameters()}
    trainable = {n for n, t in enc.named_parameters() if t.requires_grad}
    R = torch.randn((len(graph.a_scope), hidden), generator=torch.Generator().manual_seed(b))
    enc = enc.to(DEV)
    out = enc(graph)
    saved = mpn.saved_preactivations(out)
    kinks = {'Z': [z.cpu() > 0 for z in saved['Z']], 'Zo': saved['Zo'].cpu() > 0}
    (out * R.to(DEV)).sum().backward()
    hip = {'output': out.detach().cpu().numpy()}
    hip.update({n: t.grad.cpu().numpy() for n, t in enc.named_parameters() if t.grad is not None})
    ref64 = _reference(cpu, trainable, graph, args, R, torch.float64, kinks)
    ref32 = _reference(cpu, trainable, graph, args, R, torch.float32, kinks)
    assert hip.keys() == ref64.keys() == ref32.keys()
    e_hip = {n: golden_io.normwise(hip[n], ref64[n]) for n in ref64}
    e32 = {n: golden_io.normwise(ref32[n], ref64[n]) for n in ref64}
    e_hip['output rows'], e32['output rows'] = _rows(hip['output'], ref64['output']), _rows(ref32['output'], ref64['output'])
    bad = {}
    print(f'\n{name}')
    for n in e_hip:
        base = max(e32[n], e32['output'])
        print(f'  {n:20s} e_hip {e_hip[n]:.2e}  e32 {e32[n]:.2e}  e_hip / max(e32, e32 output) {e_hip[n] / base:.2f}')
        if not e_hip[n] <= FACTOR * base:
            bad[n] = (e_hip[n], base)
    assert not bad, bad
