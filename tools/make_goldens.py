"""Generate the golden fixtures under tests/golden/ from the REAL reference hot path.

Run in the build container only (needs /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_goldens.py [case ...]   (default: every case)

For each case: synthetic featurised graphs (chemprop_amd.synthetic, seeded) are fed into the
reference ``BatchMolGraph`` (featurization.py:757-813) and ``MPNEncoder`` / ``MoleculeModel``
(mpn.py:14-173, model.py:14-194) with parameters from ``synthetic_parameter`` (regenerated from the
seed by the tests, so weights are not stored).  Stored: the per-molecule graphs, the reference's
packed index arrays (a2b/b2a/b2revb/scopes), the output, and gradients of sum(out * R) for a seeded R.
Dropout is 0 everywhere (torch's dropout RNG cannot be matched).
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'polymer-chemprop_amd'))

from ref_loader import load_reference  # noqa: E402
from chemprop_amd import synthetic  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')

BASE_ARGS = dict(atom_messages=False, hidden_size=300, bias=False, depth=3, dropout=0.0, undirected=False,
                 device=torch.device('cpu'), aggregation='mean', aggregation_norm=100, activation='ReLU',
                 atom_descriptors=None, atom_descriptors_size=0, features_only=False,
                 use_input_features=False, overwrite_default_atom_features=False,
                 overwrite_default_bond_features=False, mpn_shared=False, number_of_molecules=1,
                 dataset_type='regression', num_tasks=1, multiclass_num_classes=3, checkpoint_frzn=None,
                 ffn_num_layers=2, ffn_hidden_size=None, features_size=0, spectra_activation='exp')

# name -> (graph spec, arg overrides, level, store grads)
CASES = {
    'enc_polymer_h300_t3': (('polymer', 4, 11), {}, 'encoder', True),
    'enc_polymer_bias_leaky_sum': (('polymer', 6, 12), dict(hidden_size=64, bias=True, activation='LeakyReLU',
                                                           aggregation='sum'), 'encoder', True),
    'enc_polymer_undirected_tanh_norm': (('polymer', 4, 13), dict(hidden_size=48, depth=4, undirected=True,
                                                                 activation='tanh', aggregation='norm'),
                                         'encoder', True),
    'enc_polymer_prelu_bias_t2': (('polymer', 4, 14), dict(hidden_size=40, depth=2, bias=True,
                                                          activation='PReLU'), 'encoder', True),
    'enc_qm9_selu': (('qm9', 8, 15), dict(hidden_size=32, activation='SELU'), 'encoder', True),
    'enc_edge_cases_elu_bias': (('edge', 5, 16), dict(hidden_size=64, bias=True, activation='ELU'),
                                'encoder', True),
    'enc_atom_messages': (('polymer', 4, 17), dict(hidden_size=32, atom_messages=True), 'encoder', True),
    'enc_atom_messages_bias_sum': (('polymer', 3, 18), dict(hidden_size=32, atom_messages=True, bias=True,
                                                           aggregation='sum'), 'encoder', True),
    'enc_descriptors': (('polymer', 3, 19), dict(hidden_size=32, atom_descriptors='descriptor',
                                                 atom_descriptors_size=8), 'encoder', True),
    'enc_depth1': (('polymer', 3, 20), dict(hidden_size=32, depth=1), 'encoder', True),
    'enc_undirected_bias_edge': (('edge', 5, 21), dict(hidden_size=32, depth=3, undirected=True, bias=True),
                                 'encoder', True),
    'enc_zinc_h512_t5': (('zinc', 4, 22), dict(hidden_size=512, depth=5), 'encoder', False),
    # the benchmark's batch size (polymer B = 64, H = 300, T = 3) from the real reference
    'enc_polymer_b64_h300_t3': (('polymer', 64, 31), {}, 'encoder', True),
    # QM9 B = 64 at the benchmark width: its no-grad call runs the one-launch small-block forward
    'enc_qm9_b64_h300_t3': (('qm9', 64, 32), {}, 'encoder', False),
    # zero and unit rule weights, hubs around the ELL width, a zero atom weight, Xn != 1 (synthetic.weight_case_batch):
    # the oracle's treatment of those values is the reference's own; the no-grad call is the one-launch forward
    'enc_weights_h300_t3': (('weights', 14, 33), dict(bias=True), 'encoder', True),
    'model_polymer_regression': (('polymer', 5, 23), dict(hidden_size=64, ffn_hidden_size=64), 'model', True),
    'model_two_mols_features_cls': (('polymer2', 4, 24), dict(hidden_size=32, ffn_hidden_size=16, ffn_num_layers=3,
                                                              number_of_molecules=2, use_input_features=True,
                                                              features_size=5, dataset_type='classification',
                                                              num_tasks=2), 'model', True),
    # extra atom / bond features in the reference's concatenating mode (set_extra_atom_fdim(3), set_extra_bond_fdim(2);
    # widened synthetic graphs, synthetic.with_extra_features): written to tests/golden/extra_features/
    'enc_extra_features': (('polymer', 4, 34), dict(hidden_size=32, bias=True, extra_features=(3, 2)), 'encoder', True),
}


def make_graphs(kind, b, seed):
    if kind == 'edge':
        return [synthetic.edge_case_batch(seed)]
    if kind == 'weights':
        return [synthetic.weight_case_batch(seed)]
    if kind == 'polymer2':
        return [synthetic.make_batch('polymer', b, seed), synthetic.make_batch('qm9', b, seed + 1000)]
    return [synthetic.make_batch(kind, b, seed)]


def pack_mols(prefix, graphs, out, fa_w=133, fb_w=147):
    """Per-molecule MolGraph arrays (local indices), concatenated with counts."""
    out[f'{prefix}n_atoms'] = np.array([g.n_atoms for g in graphs], np.int64)
    out[f'{prefix}n_bonds'] = np.array([g.n_bonds for g in graphs], np.int64)
    fa = [np.asarray(g.f_atoms, np.float32).reshape(g.n_atoms, fa_w) for g in graphs]
    fb = [np.asarray(g.f_bonds, np.float32).reshape(g.n_bonds, fb_w) for g in graphs]
    out[f'{prefix}f_atoms'] = np.concatenate(fa)
    out[f'{prefix}f_bonds'] = np.concatenate(fb)
    out[f'{prefix}w_atoms'] = np.concatenate([np.asarray(g.w_atoms, np.float32) for g in graphs])
    out[f'{prefix}w_bonds'] = np.concatenate([np.asarray(g.w_bonds, np.float32) for g in graphs])
    out[f'{prefix}b2a'] = np.concatenate([np.asarray(g.b2a, np.int64) for g in graphs])
    out[f'{prefix}b2revb'] = np.concatenate([np.asarray(g.b2revb, np.int64) for g in graphs])
    a2b_len, a2b_idx = [], []
    for g in graphs:
        for lst in g.a2b:
            a2b_len.append(len(lst))
            a2b_idx.extend(lst)
    out[f'{prefix}a2b_len'] = np.array(a2b_len, np.int64)
    out[f'{prefix}a2b_idx'] = np.array(a2b_idx, np.int64)
    out[f'{prefix}degree_of_polym'] = np.array([g.degree_of_polym for g in graphs], np.float64)


def main():
    ref = load_reference()
    os.makedirs(OUT, exist_ok=True)
    only = set(sys.argv[1:])
    for name, ((kind, b, seed), overrides, level, grads) in CASES.items():
        if only and name not in only:
            continue
        overrides = dict(overrides)
        da, db = overrides.pop('extra_features', (0, 0))
        args = types.SimpleNamespace(**{**BASE_ARGS, **overrides})
        if args.ffn_hidden_size is None:
            args.ffn_hidden_size = args.hidden_size
        torch.manual_seed(0)
        mol_lists = make_graphs(kind, b, seed)
        if da or db:
            mol_lists = [synthetic.with_extra_features(gs, da, db, seed) for gs in mol_lists]
        ref.featurization.set_extra_atom_fdim(da)
        ref.featurization.set_extra_bond_fdim(db)
        batches = [ref.featurization.BatchMolGraph(gs) for gs in mol_lists]
        out = {'config': np.array(json.dumps({k: v for k, v in vars(args).items() if k != 'device'})),
               'level': np.array(level), 'param_seed': np.array(seed), 'n_slots': np.array(len(batches))}
        desc = None
        if args.atom_descriptors == 'descriptor':
            desc = synthetic.random_descriptors(mol_lists[0], args.atom_descriptors_size, seed)
            out['descriptors'] = np.concatenate(desc)
        features = None
        if args.use_input_features:
            frng = np.random.default_rng(seed + 7)
            features = [frng.standard_normal(args.features_size).astype(np.float32)
                        for _ in range(len(mol_lists[0]))]
            out['features'] = np.stack(features)
        for s, (gs, bmg) in enumerate(zip(mol_lists, batches)):
            pack_mols(f's{s}_mol_', gs, out, 133 + da, 147 + da + db)
            out[f's{s}_a2b'] = bmg.a2b.numpy()
            out[f's{s}_b2a'] = bmg.b2a.numpy()
            out[f's{s}_b2revb'] = bmg.b2revb.numpy()
            out[f's{s}_a_scope'] = np.array(bmg.a_scope, np.int64).reshape(-1, 2)
            out[f's{s}_b_scope'] = np.array(bmg.b_scope, np.int64).reshape(-1, 2)
            out[f's{s}_max_num_bonds'] = np.array(bmg.max_num_bonds)
        if level == 'encoder':
            fdim_b = ref.featurization.get_bond_fdim(atom_messages=args.atom_messages)
            module = ref.mpn.MPNEncoder(args, ref.featurization.get_atom_fdim(), fdim_b)
            synthetic.fill_parameters(module, seed)
            module.eval()
            y = module(batches[0], desc)
        else:
            module = ref.model.MoleculeModel(args)
            synthetic.fill_parameters(module, seed)
            module.eval()
            y = module(batches, features)
        out['output'] = y.detach().numpy()
        if grads:
            r = np.random.default_rng(seed + 99).standard_normal(tuple(y.shape)).astype(np.float32)
            out['R'] = r
            (y * torch.from_numpy(r)).sum().backward()
            for pname, p in module.named_parameters():
                if p.grad is not None:
                    out[f'grad/{pname}'] = p.grad.numpy()
        out['param_names'] = np.array(json.dumps([n for n, _ in module.named_parameters()]))
        path = os.path.join(OUT, f'{name}.npz')
        if da or db:  # (beside the top-level fixtures, which the parametrised parity tests enumerate at 133 / 147 columns)
            out['extra_dims'] = np.array([da, db], np.int64)
            os.makedirs(os.path.join(OUT, 'extra_features'), exist_ok=True)
            path = os.path.join(OUT, 'extra_features', f'{name}.npz')
        np.savez_compressed(path, **out)
        print(f'{name}: out {tuple(y.shape)} |y|max={float(y.detach().abs().max()):.4g} '
              f'{os.path.getsize(path) / 1024:.0f} KiB')


if __name__ == '__main__':
    main()
