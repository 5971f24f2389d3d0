"""The subset of ``chemprop.args.TrainArgs`` (args.py:219-650) that the hot path and the model head
read, with the reference's defaults.  Any object with these attributes (e.g. a
real reference ``TrainArgs``) can be passed instead."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import torch


@dataclass
class TrainArgs:
    # MPNEncoder (mpn.py:24-64)
    atom_messages: bool = False          # args.py:323
    hidden_size: int = 300               # args.py:312
    bias: bool = False                   # args.py:310
    depth: int = 3                       # args.py:314
    dropout: float = 0.0                 # args.py:319
    undirected: bool = False             # args.py:325
    activation: str = 'ReLU'             # args.py:321
    aggregation: str = 'mean'            # args.py:356
    aggregation_norm: int = 100          # args.py:358
    atom_descriptors: Optional[str] = None
    atom_descriptors_size: int = 0
    atom_descriptors_path: Optional[str] = None      # args.py:99 (the .npz of per-molecule descriptor arrays)
    no_atom_descriptor_scaling: bool = False         # args.py:236
    # extra atom / bond features appended to the f_atoms / f_bonds rows (atom_descriptors == 'feature',
    # --bond_features_path): the widths the encoder was built for (args.py:238-243, 590-594)
    atom_features_size: int = 0
    bond_features_size: int = 0
    bond_features_path: Optional[str] = None         # args.py:105
    no_bond_features_scaling: bool = False           # args.py:232
    device: torch.device = field(default_factory=lambda: torch.device('cuda' if torch.cuda.is_available() else 'cpu'))
    # MPN (mpn.py:189-208)
    features_only: bool = False
    use_input_features: bool = False
    overwrite_default_atom_features: bool = False
    overwrite_default_bond_features: bool = False
    mpn_shared: bool = False
    number_of_molecules: int = 1
    # MoleculeModel (model.py:23-121)
    dataset_type: str = 'regression'
    num_tasks: int = 1
    multiclass_num_classes: int = 3
    features_size: int = 0
    features_path: Optional[List[str]] = None        # args.py:85 (the files whose columns are the input features)
    no_features_scaling: bool = False                # args.py:230
    ffn_num_layers: int = 2
    ffn_hidden_size: Optional[int] = None
    spectra_activation: str = 'exp'      # args.py:413
    spectra_target_floor: float = 1e-8   # args.py:415
    alternative_loss_function: Optional[str] = None  # args.py:417 ('wasserstein', spectra only)
    spectra_phase_mask_path: Optional[str] = None    # args.py:240
    phase_features_path: Optional[str] = None        # args.py:87
    checkpoint_frzn: Optional[str] = None
    freeze_first_only: bool = False
    frzn_ffn_layers: int = 0
    frzn_encoder: bool = False           # (run_training.py:287-291's --frzn_encoder; cli.apply_freezing)
    polymer: bool = False
    ensemble_size: int = 1                           # args.py:299 (models trained by one chemprop_train run)
    task_names: Optional[List[str]] = None           # args.py:439 (the target columns; chemprop_predict's header)
    device_metrics: bool = False                     # (chemprop_train --device_metrics: evaluate.evaluate per epoch)
    fingerprint_type: str = 'MPN'                    # args.py:734 ('MPN' | 'last_FFN', chemprop_fingerprint)
    save_graph_embeddings: bool = False              # args.py:666 (chemprop_predict)
    graph_embeddings_path: Optional[str] = None      # args.py:668 (the .npy chemprop_predict writes them to)
    # optimizer (args.py:397-407, utils.py:295-310)
    init_lr: float = 1e-4
    optimizer: str = 'adam'
    weight_decay: float = 0.0

    def __post_init__(self):
        if self.ffn_hidden_size is None:  # args.py:584-585
            self.ffn_hidden_size = self.hidden_size
