/*
 * wdmpnn.h — C-ABI of the MI355X-native wD-MPNN encoder (libwdmpnn.so, gfx950).
 *
 * Drop-in boundary.  The reference (ayildiri/polymer-chemprop, pure Python/PyTorch) has no FFI for
 * this path: the hot path is the nn.Module call chain
 *
 *     MoleculeModel.forward   chemprop/models/model.py:152-194
 *       -> MPN.forward        chemprop/models/mpn.py:210-289
 *         -> MPNEncoder.forward  chemprop/models/mpn.py:66-173        (replaced by wdmpnn_forward)
 *              index_select_ND   chemprop/nn_utils.py:50-67           (replaced by wdmpnn_index_select_rows
 *                                                                      and by the CSR gathers inside forward)
 *              BatchMolGraph     chemprop/features/featurization.py:742-875 (device layout = WdGraph)
 *         autograd backward of the above (train.py:79 loss.backward)  (replaced by wdmpnn_backward)
 *
 * The Python host package (polymer-chemprop_amd/chemprop_amd) keeps the reference's Python API and
 * binds these entry points with ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions
 *  - Every pointer in WdGraph / WdParams / WdGrads is a DEVICE pointer owned by the caller (the
 *    PyTorch caching allocator).  The library never allocates device memory.
 *  - Row 0 of every atom / bond array is the reference's zero pad row (featurization.py:767-781);
 *    n_atoms / n_bonds INCLUDE it, exactly like BatchMolGraph.n_atoms / n_bonds.
 *  - fp32 storage and fp32-accurate arithmetic, int32 indices.  The GEMMs run on MFMA with fp32
 *    accumulation over exact splits of the fp32 operands: fp16 hi / lo pairs with a power-of-two scale
 *    (three products per fp32 product, the message layers and the backward's W_h GEMMs) or three bf16
 *    planes (six products: W_o, W_i and the unblocked path).  Error against fp64 stays that of an fp32
 *    GEMM; WdConfig.gemm_variant WD_VARIANT_F32 selects plain f32-in MFMA on the unblocked path.
 *  - Padding: f_atoms / f_bonds / atom_desc rows are allocated up to a multiple of 128 and their row
 *    stride covers the feature width rounded up to 32; padding is zero.  (The host packer,
 *    BatchMolGraph.device_graph, lays them out this way.)  Weights are the unpadded nn.Linear
 *    tensors; wdmpnn_pack_params builds the padded GEMM operands from them.
 *  - Return 0 on success, a negative WD_ERR_* code on argument errors, or -(hipError_t) on a HIP
 *    launch error; wdmpnn_last_error() then holds a message (thread-local).
 *  - All work is enqueued on `stream` (a hipStream_t; NULL = default stream); no host sync, no
 *    allocation, re-entrant per stream, no global mutable state besides the thread-local error.
 */
#ifndef WDMPNN_H
#define WDMPNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* (ABI 12 also covers the extra-feature fields appended at the tail of WdGraph and WdCompact: zero there means
 * "none", and every caller zero-initialises the structs, so the number did not change when they grew.) */
#define WDMPNN_ABI_VERSION 12
#define WDMPNN_ELL_WIDTH 8

enum WdActivation {     /* nn_utils.py:70-99 get_activation_function */
    WD_ACT_RELU = 0, WD_ACT_LEAKY_RELU = 1, WD_ACT_PRELU = 2, WD_ACT_TANH = 3,
    WD_ACT_SELU = 4, WD_ACT_ELU = 5, WD_ACT_IDENTITY = 6
};

enum WdAggregation {    /* mpn.py:158-163 */
    WD_AGG_MEAN = 0, WD_AGG_SUM = 1, WD_AGG_NORM = 2
};

enum WdError {
    WD_OK = 0, WD_ERR_ARG = -1000, WD_ERR_SHAPE = -1001, WD_ERR_WORKSPACE = -1002,
    WD_ERR_UNSUPPORTED = -1003
};

/* Values of WdConfig.gemm_variant (an A/B and debugging knob; any other value is not rejected). */
enum WdVariant {
    /* fp32-accurate split GEMMs with the molecule-blocked fused inference forward when
     * WdGraph.blocks allow it: its message layers and W_o read fp16 pair tiles their producers wrote (bond
     * messages, hidden rounded to 64 a multiple of 80), QM9-sized blocks take the one-launch forward */
    WD_VARIANT_DEFAULT = 0,
    /* f32-MFMA GEMMs on the unblocked path (precision A/B) */
    WD_VARIANT_F32 = 9,
    /* the fused four-launch forward also for QM9-sized blocks (no one-launch forward) */
    WD_VARIANT_FOUR_LAUNCH = 11,
    /* as FOUR_LAUNCH, the message layers staging M_{t-1} from fp32 Z_t rows through registers (the round-5
     * default); neither the packed weights nor the workspace then hold pair tiles */
    WD_VARIANT_STAGED = 12,
    /* as FOUR_LAUNCH, on pair tiles */
    WD_VARIANT_PAIRS = 13,
    /* Debug (tools/debug_pairs.py), 1ab = WD_VARIANT_DEBUG + 10 a + b: the four-launch forward with a =
     * WD_DEBUG_PAIRS pair layers or WD_DEBUG_STAGED register-staged layers (the workspace and the pack keep
     * their pair tiles either way), returning after stage b = 1 the embed, 1 + t message layer t, 0 none: the
     * intermediate buffers stay in the workspace (wdmpnn_debug_fwd_offsets).  b = WD_DEBUG_WO_DUMP at depth 3
     * (no stop left to reach) also writes the W_o pre-activation into the free second ping-pong buffer. */
    WD_VARIANT_DEBUG = 100,
    WD_DEBUG_PAIRS = 1, WD_DEBUG_STAGED = 2, WD_DEBUG_WO_DUMP = 4
};
#define WD_VARIANT_DEBUG_STOP(a, b) (WD_VARIANT_DEBUG + 10 * (a) + (b))

/* One row-gather list: row r of the gathered operand = sum_{e=ptr[r]}^{ptr[r+1]-1} coef[e] * src[idx[e]].
 * idx and coef must be readable (any value) for 8 entries past ptr[rows]: the gather kernels fetch the
 * first eight entries of a row unconditionally and discard the ones past its end. */
typedef struct WdCsr {
    const int32_t *ptr;   /* [rows + 1] */
    const int32_t *idx;   /* [ptr[rows]] source row ids */
    const float   *coef;  /* [ptr[rows]] coefficients, NULL = all ones */
} WdCsr;

/* Categorical codes of one atom / one bond pair (see "Compact graphs" below). */
typedef struct WdAtomCode {
    uint8_t col[8];         /* columns of f_atoms holding 1.0, ascending; 0xFF = unused slot     */
    float last;             /* the last column of the base block, f_atoms[atom_fdim - atom_extra_dim - 1]
                               (mass * 0.01; column 132 of the default 133)                      */
    float w;                /* w_atoms                                                           */
} WdAtomCode;
typedef struct WdBondPair {
    uint16_t a1, a2;        /* molecule-local atom ids: b1 = a1 -> a2, b2 = a2 -> a1             */
    uint16_t tail;          /* bond feature columns as bits (bit k = column atom_fdim + k)       */
    uint16_t reserved;
    float w12, w21;         /* w_bonds[b1], w_bonds[b2]                                          */
} WdBondPair;
/*
 * Device-resident packed BatchMolGraph (featurization.py:757-813) plus the gather lists derived
 * from it by the host packer (chemprop_amd/featurization.py, BatchMolGraph.device_graph()).
 */
typedef struct WdGraph {
    int32_t n_atoms;        /* V+1 (incl. pad row 0)                               */
    int32_t n_bonds;        /* E+1 (incl. pad row 0)                               */
    int32_t n_mols;         /* B = len(a_scope)                                    */
    int32_t atom_fdim;      /* Fa: columns of f_atoms actually used                */
    int32_t bond_fdim;      /* Fb: columns of f_bonds actually used (14 in atom-message mode) */
    int32_t ld_atoms;       /* row stride of f_atoms (floats)                      */
    int32_t ld_bonds;       /* row stride of f_bonds (floats)                      */
    int32_t bond_col0;      /* first used column of f_bonds (Fb_full - 14 in atom-message mode) */
    const float *f_atoms;   /* [n_atoms, ld_atoms]                                 */
    const float *f_bonds;   /* [n_bonds, ld_bonds]                                 */
    const float *w_atoms;   /* [n_atoms]  (featurization.py:778, pad weight 0)     */
    const int32_t *mol_start;  /* [B] a_scope[i][0]                                */
    const int32_t *mol_size;   /* [B] a_scope[i][1]                                */
    const float *degree_of_polym; /* [B]                                           */
    /* bond-message mode (mpn.py:110-120): X_b = sum_{j in in(b2a[b])} w_j M_j - M_{b2revb[b]} */
    WdCsr msg_gather;       /* rows = n_bonds (bond mode) or n_atoms (atom mode, a2a + pad-slot term) */
    WdCsr bond_feat_gather; /* atom mode only: rows = n_atoms, sum of f_bonds tails over a2b (mpn.py:106) */
    WdCsr atom_gather;      /* rows = n_atoms: final aggregate of mpn.py:126-131 (coef = edge weight) */
    const int32_t *b2revb;  /* [n_bonds] (undirected: mpn.py:101-102)                */
    /* transposed lists for the backward pass (gradient of the gathers) */
    WdCsr msg_gather_t;     /* rows = message rows: dM_j += sum coef * dX_row          */
    WdCsr bond_feat_gather_t; /* unused by the gradients (inputs need no grad); may be zero */
    WdCsr atom_gather_t;    /* rows = message rows: dM_j += coef * dA_atom              */
    /* atom_descriptors == 'descriptor' (mpn.py:136-143) */
    const float *atom_desc; /* [n_atoms, round32(desc_dim)] (row 0 zero pad) or NULL */
    int32_t desc_dim;
    int32_t atom_messages;  /* 1 = atom-message mode (mpn.py:47-53, 93-94, 104-108) */
    /* Optional bf16x3 plane tiles of f_atoms / f_bonds (wdmpnn_split_planes over all padded rows and
     * ld_atoms / ld_bonds columns), made once per packed graph: the exact split-plane form the bf16x6
     * GEMMs read.  NULL: those GEMMs split the fp32 features in the kernel instead. */
    const void *f_atoms_x6;
    const void *f_bonds_x6;
    /* Optional molecule blocks for the fused inference forward: consecutive molecules
     * grouped into blocks of <= 128 bond rows, <= 64 atom rows and <= 64 molecules, so that every gather
     * stays inside one block.  blocks[8 * k .. 8 * k + 5] = {bond_start, bond_count, atom_start, atom_count, mol_lo,
     * mol_hi} (natural row ids, half-open molecule range).  bond_blk_row[r] (r < rows of f_bonds) =
     * 128 * block + (r - bond_start) or -1; f_atoms_blk_x6 = plane tiles of f_atoms in the blocked atom
     * layout (row 64 * block + (a - atom_start), zero rows elsewhere).  n_blocks = 0: unavailable. */
    int32_t n_blocks;
    const int32_t *blocks;
    const int32_t *bond_blk_row;
    const void *f_atoms_blk_x6;
    /* Required with blocks: the first WDMPNN_ELL_WIDTH (W = 8) entries of every msg_gather / atom_gather
     * row in block-local ELL form, so that the fused kernels prefetch a row's list with independent
     * loads during the GEMM instead of a ptr -> idx chain after it.  *_ell_idx[W r + k] = idx - the
     * first row of the gathered kind in the row's block (bond_start for bond rows; atom_start in
     * atom-message mode, whose gathers read atom rows), uint8 < 128, *_ell_coef[W r + k] = coef; unused
     * slots coef 0 and a valid index; bit 7 of slot W - 1 set when the row has more than W entries (the
     * rest are read from the CSR lists).  Atom-message mode: msg_ell lists only the real a2a entries (the
     * pad slots' atom 0 is dropped; the fused path runs bias-free models only, whose pad messages are 0),
     * and the CSR rest of a longer row skips entries outside the block. */
    const uint8_t *msg_ell_idx;
    const float *msg_ell_coef;
    const uint8_t *atom_ell_idx;
    const float *atom_ell_coef;
    /* Optional categorical codes (compact graphs, wdmpnn_build_graph; NULL otherwise).  With blocks, the
     * fused forward then replaces the W_i GEMM and the f_atoms half of the W_o GEMM by sums of weight
     * columns (one-hot rows: f W^T = sum of the columns holding 1.0 + last * the last column):
     * atom_codes [n_atoms] natural rows; bond_src_blk [rows of f_bonds] = the block-local index of the
     * bond's source atom (b2a); bond_tail [rows of f_bonds] = its bond columns as bits. */
    const WdAtomCode *atom_codes;
    const uint8_t *bond_src_blk;
    const uint16_t *bond_tail;
    /* Optional, atom-message mode (ABI 8): per atom row the sum of its in-bonds' feature rows
     * (bond_feat_gather applied to f_bonds, mpn.py:105-106 summed over the slots: a function of the graph
     * alone) as bf16x3 plane tiles [rows of f_atoms][ld_bonds], made with the graph's other planes.  NULL:
     * the fused forward gathers it in one extra launch. */
    const void *atom_feat_sum_x6;
    /* Optional (ABI 9): the largest bond / atom row counts of any block (0 = unknown).  When every block
     * holds <= 32 of each (QM9-sized molecules) the fused inference forward runs as ONE launch, a
     * workgroup carrying its block from the input layer to the readout (small_fwd.hpp). */
    int32_t blk_max_bonds;
    int32_t blk_max_atoms;
    /* Optional, with atom_codes (appended under ABI 12; 0 / NULL = none): extra atom / bond features, the dense
     * tail of the rows (featurization.py:436-440, 460-468: f_atoms = [base | atom_extra], f_bonds = [f_atoms[src] |
     * bond bits | bond_extra]).  atom_extra [n_atoms][atom_extra_dim] natural atom rows (pad row 0 zero);
     * bond_extra [(n_bonds - 1) / 2][bond_extra_dim] one row per bond pair, so directed bond b reads row
     * (b - 1) >> 1.  atom_fdim / bond_fdim include them; the codes' columns and WdAtomCode.last address the base
     * block of atom_fdim - atom_extra_dim columns.  The fused forward's embed adds them as a dense tail. */
    const float *atom_extra;
    const float *bond_extra;
    int32_t atom_extra_dim;
    int32_t bond_extra_dim;
} WdGraph;

/* nn.Module parameters of MPNEncoder (mpn.py:17-64); all device pointers, row-major like nn.Linear. */
typedef struct WdParams {
    int32_t hidden;         /* H = args.hidden_size                                */
    const float *W_i;       /* [H, Kin], Kin = bond_fdim (bond mode) or atom_fdim */
    const float *b_i;       /* [H] or NULL (args.bias)                             */
    const float *W_h;       /* [H, H] (bond mode) or [H, H + bond_fdim] (atom mode) */
    const float *b_h;       /* [H] or NULL                                         */
    const float *W_o;       /* [H, atom_fdim + H]                                  */
    const float *b_o;       /* [H] (always present, mpn.py:58)                     */
    const float *W_d;       /* [H+d, H+d] atom_descriptors_layer or NULL          */
    const float *b_d;       /* [H+d] or NULL                                       */
    const float *prelu;     /* [1] PReLU slope (device) when activation == PReLU   */
    const float *zero_vec;  /* [H] cached_zero_vector (mpn.py:44, 148-149)         */
    const void  *packed;    /* optional: output of wdmpnn_pack_params for these weights; NULL =
                               wdmpnn_forward packs into its own workspace (one extra launch)     */
    size_t packed_bytes;
} WdParams;

typedef struct WdConfig {
    int32_t depth;          /* args.depth (>= 1)                                   */
    int32_t undirected;     /* args.undirected                                     */
    int32_t activation;     /* WdActivation                                        */
    int32_t aggregation;    /* WdAggregation                                       */
    float   aggregation_norm;
    float   dropout;        /* args.dropout; 0 at eval                             */
    uint64_t seed;          /* dropout RNG stream (counter based, re-derivable in backward) */
    int32_t save_for_backward; /* 1: keep pre-activations + every message layer in the workspace */
    int32_t prof_slot;      /* first event pair used when prof_pool != NULL                      */
    void   *prof_pool;      /* optional WdEventPool: one event pair (pair prof_slot) is recorded around
                               the depth - 1 message-passing launches (the dominant kernel) of this
                               forward: before the first, after the last                          */
    int32_t gemm_variant;   /* WdVariant (0 = WD_VARIANT_DEFAULT)                                      */
} WdConfig;

/* Gradients (device, caller-zeroed NOT required: every pointer is fully overwritten). NULL = skip. */
typedef struct WdGrads {
    float *W_i, *b_i, *W_h, *b_h, *W_o, *b_o, *W_d, *b_d, *prelu;
} WdGrads;

int wdmpnn_abi_version(void);
const char *wdmpnn_last_error(void);
/* Load-time kernel check (ABI 11): 0 when the library's gfx950 code object holds every kernel its host
 * code launches (a mismatched build would otherwise abort the process inside a HIP launch), else
 * WD_ERR_UNSUPPORTED with the missing kernel in wdmpnn_last_error().  Reads only the library file (no HIP
 * call, runs without a GPU); every compute entry point runs it once per process and fails the same way.
 * The counts (either pointer may be NULL): kernels the host registers, kernel descriptors in the code
 * object. */
int wdmpnn_self_check(int32_t *n_host_kernels, int32_t *n_device_kernels);

/* Padded / transposed copies of the weights for the GEMMs; depends only on the parameter values and
 * the encoder dimensions, so callers cache it per parameter version (chemprop_amd does). */
int wdmpnn_packed_params_bytes(const WdGraph *g, const WdParams *p, const WdConfig *c, size_t *bytes);
int wdmpnn_pack_params(const WdGraph *g, const WdParams *p, const WdConfig *c, void *packed, size_t bytes,
                       void *stream);

/* Bytes of forward workspace (intermediates kept for backward when save_for_backward). */
int wdmpnn_workspace_bytes(const WdGraph *g, const WdParams *p, const WdConfig *c, size_t *bytes);
/* Bytes of scratch for wdmpnn_backward. */
int wdmpnn_backward_workspace_bytes(const WdGraph *g, const WdParams *p, const WdConfig *c, size_t *bytes);

/* MPNEncoder.forward (mpn.py:66-173): out [n_mols, H (+desc_dim)]. */
int wdmpnn_forward(const WdGraph *g, const WdParams *p, const WdConfig *c,
                   void *workspace, size_t workspace_bytes, float *out, void *stream);

/* Several independent batches through the fused inference forward in one set of launches: the embed,
 * the depth - 1 message-passing layers and W_o + readout each run ONCE for up to 8 batches (their tiles
 * concatenated in one grid), instead of once per batch.  Replaces a loop of MPNEncoder.forward calls
 * over batches (the caller of chemprop/train/predict.py:30-40 issues one forward per batch) for batches
 * that are ready together; batch j's output equals wdmpnn_forward(graphs[j], ...) bitwise.
 * graphs[j]: each a molecule-blocked graph (WdGraph.blocks; compact-code or host-built), same feature
 * sizes; p->packed must hold the packed parameters (wdmpnn_pack_params); c->save_for_backward = 0;
 * workspaces[j] of wdmpnn_workspace_bytes(graphs[j], ...) bytes; outs[j] [n_mols_j, H].  Any n >= 0
 * (chunks of 8 per launch set). */
int wdmpnn_forward_many(int32_t n, const WdGraph *graphs, const WdParams *p, const WdConfig *c,
                        void *const *workspaces, const size_t *workspace_bytes, float *const *outs, void *stream);

/* Gradient of MPNEncoder.forward w.r.t. its parameters, given dout [n_mols, H (+desc_dim)] and the
 * workspace of a forward run with save_for_backward = 1 and identical g/p/c. */
int wdmpnn_backward(const WdGraph *g, const WdParams *p, const WdConfig *c,
                    const void *workspace, size_t workspace_bytes, const float *dout,
                    void *scratch, size_t scratch_bytes, const WdGrads *grads, void *stream);

/* Introspection of a save_for_backward forward's workspace (tests, debugging): byte offsets of the
 * saved fp32 pre-activations.  Z_t (t = 0 .. depth-1) = the input of the activation of message layer t
 * (t = 0: W_i, mpn.py:96-97; t >= 1: mpn.py:123), [rows][ld] in natural row order; zo = the W_o
 * pre-activation (mpn.py:133), [atom_rows][ld].  Padding rows / columns hold 0. */
#define WDMPNN_MAX_SAVED_DEPTH 32
typedef struct WdSaved {
    int32_t depth, rows, atom_rows, ld;
    size_t z[WDMPNN_MAX_SAVED_DEPTH];
    size_t zo;
} WdSaved;
int wdmpnn_saved_layout(const WdGraph *g, const WdParams *p, const WdConfig *c, WdSaved *out);

/* Measurement hook (bench.py): a pool of hipEvent pairs recorded by wdmpnn_forward around its
 * dominant launches (see WdConfig.prof_pool).  elapsed_ms synchronises on the events it reads. */
int wdmpnn_event_pool_create(int32_t n_pairs, void **pool);
int wdmpnn_event_pool_destroy(void *pool);
int wdmpnn_event_pool_elapsed_ms(void *pool, int32_t first, int32_t count, float *total_ms);

/* bf16x3 plane tiles of the first kp columns of an fp32 [rows, ld] matrix (rows % 64 == 0,
 * kp % 32 == 0, ld >= kp, ld % 4 == 0): the layout of WdGraph.f_atoms_x6 / f_bonds_x6.  The planes hold
 * every fp32 value exactly (x = h + m + l).  plane_bytes = rows * kp * 6. */
int wdmpnn_plane_bytes(int32_t rows, int32_t kp, size_t *bytes);
int wdmpnn_split_planes(const float *src, int32_t ld, int32_t rows, int32_t kp, void *dst, size_t dst_bytes,
                        void *stream);
/* The same with a row map: source row r goes to plane-tile row row_map[r] (skipped when < 0) of a
 * [out_rows, kp] plane-tile matrix whose other rows are zero-filled.  Every row_map[r] must be < out_rows: the
 * device does not check it. */
int wdmpnn_split_planes_rows(const float *src, int32_t ld, int32_t rows, int32_t kp, const int32_t *row_map,
                             int32_t out_rows, void *dst, size_t dst_bytes, void *stream);

/* Device-side bond featurisation, replacing the host-side construction of every
 * f_bonds row as f_atoms[a1] + f_bond (featurization.py:467-468, 545-546, 616-617) and its H2D copy:
 * f_bonds[r][0 .. atom_fdim) = f_atoms[b2a[r]], f_bonds[r][atom_fdim .. + tail_dim) = bond_tail[r],
 * the rest of the ld_bonds columns 0, for r < rows.  b2a entries must index f_atoms rows
 * (< atom_rows); an out-of-range entry fills its row's atom part with NaN. */
int wdmpnn_build_bond_features(const float *f_atoms, int32_t ld_atoms, int32_t atom_fdim, int32_t atom_rows,
                               const int32_t *b2a, const float *bond_tail, int32_t ld_tail, int32_t tail_dim,
                               int32_t rows, float *f_bonds, int32_t ld_bonds, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Compact graphs: categorical codes on the wire, the whole WdGraph built on the device
 * (SURVEY §8(f) row 2).
 *
 * The reference featurises every atom as six one-hot blocks + an aromatic bit + mass * 0.01
 * (featurization.py:190-211, 133 columns) and every bond as 14 binary columns (featurization.py:229-250);
 * each directed bond row is its source atom's row followed by the bond's (featurization.py:467-468,
 * 545-546, 616-617), and MolGraph appends bonds in pairs b1 = a1 -> a2, b2 = a2 -> a1 = b2revb[b1]
 * (featurization.py:469-480, 621-630), a2b[a] listing the bonds INTO a in creation order.  A batch in
 * that form travels as
 *   WdAtomCode [n_atoms]  the columns holding 1.0 (ascending, 0xFF = none) + the last column's value
 *                         (mass * 0.01) + the atom weight (w_atoms, featurization.py:507);
 *   WdBondPair [pairs]    molecule-local endpoints a1, a2, the 14 bond columns as a bit mask (bit k =
 *                         column atom_fdim + k) and the two directed weights (w_bonds, :628);
 *   mols [n_mols][4]      {atom_start, n_atoms, bond_start, n_bonds} (natural ids, pad row 0 included
 *                         in the numbering like BatchMolGraph.a_scope / b_scope) + xn [n_mols];
 *   blocks [n_blocks][8]  the molecule blocks of the fused forward (WdGraph.blocks) + block_nnz
 *                         [n_blocks][2] = {first msg_gather entry, first atom_gather entry} of the block;
 * about 14 bytes per directed edge, against ~450 for the fp32 rows + gather lists.  wdmpnn_build_graph
 * expands it on the device into every WdGraph array (fp32 feature rows, plane tiles, gather lists and
 * their transposes, ELL rows, block maps) with the same values and entry order as the host packer
 * (chemprop_amd.featurization.BatchMolGraph.device_graph): one launch.  Requires every molecule to fit
 * one block (<= 128 directed bonds, <= 64 atoms); atom_fdim <= 255 with the code's columns < atom_fdim - 1.
 * ------------------------------------------------------------------------------------------------ */
typedef struct WdCompact {
    int32_t n_mols, n_atoms, n_bonds, n_blocks;   /* n_atoms / n_bonds include the pad row        */
    int32_t atom_fdim, bond_fdim;                 /* 133 / 147 by default (bond_fdim - atom_fdim - bond_extra_dim <= 16) */
    int32_t nnz_msg, nnz_agg;                     /* total entries of msg_gather / atom_gather    */
    const int32_t *mols;                          /* [n_mols][4]                                  */
    const float *xn;                              /* [n_mols] degree_of_polym                     */
    const WdAtomCode *atoms;                      /* [n_atoms], row 0 = pad (no columns, 0, 0)    */
    const WdBondPair *pairs;                      /* [(n_bonds - 1) / 2]                          */
    const int32_t *blocks;                        /* [n_blocks][8]                                */
    const int32_t *block_nnz;                     /* [n_blocks][2]                                */
    /* Extra atom / bond features (appended under ABI 12; 0 / NULL = none): atom_fdim and bond_fdim include them,
     * bond_fdim - atom_fdim - bond_extra_dim <= 16 are the bit columns, each dim <= 64.  atom_extra [n_atoms]
     * [atom_extra_dim] fp32 natural rows (pad row 0 zero), bond_extra [(n_bonds - 1) / 2][bond_extra_dim] fp32
     * one row per WdBondPair (both directed bonds carry the same values). */
    int32_t atom_extra_dim, bond_extra_dim;
    const float *atom_extra;
    const float *bond_extra;
} WdCompact;

/* Device bytes of the graph wdmpnn_build_graph writes (one buffer, caller-allocated). */
int wdmpnn_graph_bytes(const WdCompact *c, size_t *bytes);
/* Build the WdGraph of a compact batch into `buffer` (device, >= wdmpnn_graph_bytes, 256-byte aligned)
 * on `stream`; *g receives the struct (bond-message mode, blocks set, no descriptors) whose pointers
 * point into `buffer`.  All arrays of c are device pointers. */
int wdmpnn_build_graph(const WdCompact *c, void *buffer, size_t bytes, WdGraph *g, void *stream);
/* The same with flags.  WDMPNN_GRAPH_LEAN: skip the dense feature rows, their plane tiles, the bond
 * message gathers and the transposed gathers (most of the bytes written for a polymer batch); the graph
 * then serves only the fused inference forward (categorical codes) -- anything else returns
 * WD_ERR_UNSUPPORTED. */
#define WDMPNN_GRAPH_LEAN 1
/* WDMPNN_GRAPH_NO_PLANES: skip only the bf16 plane tiles of the feature rows (f_atoms_x6, f_bonds_x6,
 * f_atoms_blk_x6 stay NULL).  The fused forward and backward of a categorical-code graph never read them
 * (training streams); unblocked paths fall back to their register-split GEMMs. */
#define WDMPNN_GRAPH_NO_PLANES 2
int wdmpnn_build_graph_ex(const WdCompact *c, void *buffer, size_t bytes, WdGraph *g, int32_t flags, void *stream);

/* Atom-message mode (WdGraph.atom_messages = 1; mpn.py:47-53, 93-94, 104-108, 126-128) from the same compact
 * image and block plan: one launch, one workgroup per molecule block and slice + one for the pad rows.
 * Message rows are atoms and every list's row a has deg(a) entries (msg_gather: deg(a) + 1), so every offset
 * follows from the block table alone: c->nnz_msg, c->nnz_agg and c->block_nnz are not read (a resident table
 * needs no per-batch entry counts).  max_num_bonds = the batch's largest atom degree (>= 1,
 * BatchMolGraph.max_num_bonds).  With Fb' = c->bond_fdim - c->atom_fdim the graph holds
 *   f_atoms (+ natural and molecule-blocked planes), w_atoms, the scope arrays, b2revb, blocks, bond_blk_row
 *                      as wdmpnn_build_graph writes them (atom extras included);
 *   f_bonds [.][rup(Fb', 32)]  the bond's own columns: the bit columns, then bond_extra[pair]; bond_fdim = Fb';
 *   bond_feat_gather   row a = the bonds into a in creation order, coefficient 1;
 *   atom_feat_sum_x6   planes of sum_{j in in(a)} f_bonds[j], fp32, added in list order;
 *   msg_gather         row a = (b2a[j], 1) for j in in(a), then ONE pad entry (0, max_num_bonds - deg(a)),
 *                      written even when the coefficient is 0; row 0 = (0, max_num_bonds);
 *   atom_gather        row a = (b2a[j], w_bonds[b2a[j]]) for j in in(a): the reference's quirk (mpn.py:128), the
 *                      weight looked up by the ATOM id used as a bond id; zero coefficients are kept, and an id
 *                      past the bonds reads 0 (callers route such batches to the host packer);
 *   msg_gather_t, atom_gather_t   the exact transposes over atom rows, entries by increasing forward row, then
 *                      position; msg_gather_t row 0 = the n_atoms pad entries;
 *   msg_ell_*, atom_ell_*   per atom: the first 8 real a2a entries (pad entry dropped) / the first 8 atom_gather
 *                      entries, block-local atom indices, bit 7 of slot 7 set when deg(a) > 8.
 * atom_codes, bond_src_blk, bond_tail, atom_extra and bond_extra stay NULL.  After dropping zero coefficients
 * every list equals the host packer's entry for entry, so outputs and gradients are bitwise the host-built
 * graph's.  Buffer contract as wdmpnn_build_graph (256-byte aligned, WD_ERR_WORKSPACE when short); no lean
 * variant, no batching of several builds per launch. */
int wdmpnn_graph_bytes_atom(const WdCompact *c, size_t *bytes);
int wdmpnn_build_graph_atom(const WdCompact *c, void *buffer, size_t bytes, WdGraph *g, int32_t max_num_bonds,
                            void *stream);

/* Resident graph tables: the compact image of a batch assembled on the device from the codes of a whole data
 * split, uploaded once per run (chemprop_amd.graph_table).  A molecule's compact record is position-independent
 * (WdAtomCode holds nothing batch-relative, WdBondPair.a1 / a2 are molecule-local), so the xn, atoms and pairs
 * sections of the image of any batch are a segmented copy of per-molecule records; mols, blocks and block_nnz
 * are the small host plan (csrc/compact.hpp plan_sizes, from the molecules' sizes and entry counts alone).
 *
 * The table: t_atoms and t_pairs hold every molecule's records back to back (no pad rows), t_xn its
 * degree_of_polym, t_first [molecules][2] (int64, so a table of millions of molecules does not overflow) the
 * index of its first atom record and of its first pair record.  A table of rows of n_slots molecules
 * (number_of_molecules > 1) numbers its molecules row * n_slots + slot.
 * The batch: ids [n_rows] (int64) are table rows, a slice of an index that was validated on the host; batch
 * molecule m, m < n_mols, is slot slot0 + m / n_rows of row ids[m % n_rows].  A batch of one slot has
 * n_mols = n_rows; the merged batch of a shared encoder (slot 0's molecules, then slot 1's, ...) has
 * n_mols = n_slots * n_rows and slot0 = 0.  Repeated ids, or ids in any order, give the corresponding copies.
 * The destination: the sections of an image laid out as the staged upload image (mols | xn | atoms | pairs |
 * blocks | block_nnz); mols [n_mols][4] must already be there (uploaded earlier on the same stream) and must
 * give every molecule the sizes its table record has.  One launch writes
 *     atoms[0]                                 the pad row (no columns, last = 0, w = 0)
 *     atoms[atom_start_m + i]                = t_atoms[first atom record + i]     i < n_atoms_m
 *     pairs[(bond_start_m - 1) / 2 + i]      = t_pairs[first pair record + i]     i < n_bonds_m / 2
 *     xn[m]                                  = t_xn[molecule]
 * and with the host plan's three sections the image is bitwise the one the host stages for the same molecules
 * in the same order, so the graph built from it and everything downstream are bitwise unchanged.
 * One wave per molecule, a 128-bit load and a 128-bit store per record per lane; no atomics, no LDS, plain
 * vector stores, a fixed thread-to-record map.  The kernel clamps nothing, like the row join above: range
 * checking of ids is the caller's (chemprop_amd.graph_table.GraphTable.index).
 * Refused before any launch: a NULL struct, or with n_mols > 0 one of the nine pointers NULL or one of t_atoms,
 * t_pairs, mols, atoms, pairs off a 16-byte boundary (WD_ERR_ARG);
 * n_mols < 0, n_rows < 0, or with n_mols > 0: n_rows < 1, n_slots < 1, slot0 < 0, n_mols not a multiple of
 * n_rows, slot0 + n_mols / n_rows > n_slots (WD_ERR_SHAPE).  n_mols == 0 is a no-op. */
typedef struct WdGatherCompact {
    int32_t n_mols, n_rows, n_slots, slot0;
    const WdAtomCode *t_atoms;    /* table: atom records of every molecule                  */
    const WdBondPair *t_pairs;    /* table: pair records of every molecule                  */
    const float *t_xn;            /* table: [molecules] degree_of_polym                     */
    const int64_t *t_first;       /* table: [molecules][2] first atom / first pair record   */
    const int64_t *ids;           /* [n_rows] table rows                                    */
    const int32_t *mols;          /* image: [n_mols][4], already uploaded                   */
    float *xn;                    /* image: [n_mols]                                        */
    WdAtomCode *atoms;            /* image: [1 + sum n_atoms]                               */
    WdBondPair *pairs;            /* image: [sum n_bonds / 2]                               */
} WdGatherCompact;
int wdmpnn_gather_compact(const WdGatherCompact *g, void *stream);

/* index_select_ND (nn_utils.py:50-67): out[i, :] = src[index[i], :], row_len floats per row.
 * Indices are int64 like the reference's LongTensor; out-of-range indices are an error checked by
 * the caller (the kernel clamps nothing and reads src[index]). */
int wdmpnn_index_select_rows(const float *src, int64_t n_src_rows, int64_t row_len,
                             const int64_t *index, int64_t n_index, float *out, void *stream);
/* Its gradient (the backward of nn_utils.py:64's index_select under autograd): dsrc[j, :] = sum of
 * grad[p, :] over the positions p with index[p] == j, in increasing p (deterministic, no atomics).
 * perm [n_index] = the positions sorted stably by index value, ptr [n_src_rows + 1] = the CSR bounds of
 * each source row in perm.  Every dsrc row is written (0 for rows never selected). */
int wdmpnn_index_select_rows_backward(const float *grad, int64_t n_index, int64_t row_len, const int64_t *perm,
                                      const int64_t *ptr, int64_t n_src_rows, float *dsrc, void *stream);

/* Join, gather or split rows: one launch builds the row-major fp32 matrix `out` [B][ld_out] from up to
 * WD_JOIN_MAX_SEGMENTS column segments, each optionally gathered by a row index:
 *     out[b][o_s + j] = src_s[(idx_s ? idx_s[b] : b) * ld_s + c0_s + j]     j < w_s,  o_s = w_0 + ... + w_{s-1}
 * Uses: the FFN input x = [encoding | feature_table[idx]] of a model with molecule features (mpn.py:281-285,
 * the torch.cat of MPN.forward) as two segments; a row gather (one segment with an index); the contiguous
 * copy of a column range, dEmb = dx[:, 0:H] (one segment, c0 = 0, ld = ld_x).
 * A pure copy: every payload bit is preserved (NaN payloads, -0.0).  Columns of `out` at and beyond the
 * sum of the widths are not written.  No atomics, a fixed thread-to-element map.  A segment moves as
 * 16-byte vectors when src, ld, c0, its destination offset, out and ld_out are all multiples of 16 bytes
 * (the last w % 4 columns as single words), else word by word.  Indices are int64 like
 * wdmpnn_index_select_rows'; the kernel clamps nothing and reads src[idx[b]]: range checking is the caller's.
 * Refused before any launch: n_seg > WD_JOIN_MAX_SEGMENTS (WD_ERR_UNSUPPORTED), n_seg < 1 or a NULL struct
 * (WD_ERR_ARG); B < 0, w <= 0, c0 < 0, ld < c0 + w, ld_out < sum of w (WD_ERR_SHAPE); out or a src NULL
 * with B > 0 (WD_ERR_ARG).  B == 0 is a no-op. */
#define WD_JOIN_MAX_SEGMENTS 4
typedef struct WdJoin {
    int32_t B, n_seg;
    struct {
        const float *src;    /* [rows][ld]                                   */
        int32_t ld, c0, w;   /* leading dimension, first column, columns     */
        const int64_t *idx;  /* [B] source rows, or NULL: row b              */
    } seg[WD_JOIN_MAX_SEGMENTS];
    float *out;              /* [B][ld_out]                                  */
    int32_t ld_out;
} WdJoin;
int wdmpnn_join_rows(const WdJoin *j, void *stream);

/* The FFN input of a model of several molecules per input (number_of_molecules > 1; mpn.py:270-285, the
 * torch.cat of the encoders' outputs and of the features) and its inverse, each one launch for any number
 * of slots up to WD_MAX_SLOTS.  wdmpnn_slots_join:
 *     x[b][k * H + j]       = slot[k][b * ld_slot + j]                              k < n_slots, j < H
 *     x[b][n_slots * H + j] = feat[(feat_idx ? feat_idx[b] : b) * ld_feat + j]      j < Ff
 * wdmpnn_slots_split: slot[k][b * ld_slot + j] = x[b][k * H + j] (the gradient of the join with respect to
 * the slots: what torch.cat's backward hands to each encoder); it ignores the feature fields.
 * Pure copies: every payload bit is preserved (NaN payloads, -0.0).  The join never writes columns of x at
 * and beyond n_slots * H + Ff.  No atomics, a fixed thread-to-element map.  Both move 16-byte vectors when x,
 * every slot pointer, feat (join with Ff > 0), ld_x, ld_slot, ld_feat (likewise) and H are all multiples of
 * 16 bytes (the last Ff % 4 feature columns as single words), else word by word.  The slot pointers may
 * point into one buffer: slot[k] = base + k * B * H with ld_slot = H is the slot-major [n_slots * B][H]
 * matrix a shared encoder writes for the merged batch of all slots.  Indices are int64 like
 * wdmpnn_join_rows'; the kernel clamps nothing and reads feat[feat_idx[b]]: range checking is the caller's.
 * Refused before any launch: n_slots > WD_MAX_SLOTS (WD_ERR_UNSUPPORTED), n_slots < 1 or a NULL struct
 * (WD_ERR_ARG); B < 0, H <= 0, ld_slot < H, Ff < 0, ld_feat < Ff, ld_x < n_slots * H + Ff (WD_ERR_SHAPE);
 * x, a slot pointer or feat (with Ff > 0) NULL with B > 0 (WD_ERR_ARG).  B == 0 is a no-op. */
#define WD_MAX_SLOTS 8
typedef struct WdSlots {
    int32_t B, n_slots, H;       /* rows, molecules per input, columns per slot          */
    float *slot[WD_MAX_SLOTS];   /* slot k: [B][ld_slot], H columns used                 */
    int32_t ld_slot;
    const float *feat;           /* join only: [rows][ld_feat], or NULL with Ff == 0     */
    int32_t ld_feat, Ff;
    const int64_t *feat_idx;     /* [B] feature rows, or NULL: row b                     */
    float *x;                    /* [B][ld_x], ld_x >= n_slots * H + Ff                  */
    int32_t ld_x;
} WdSlots;
int wdmpnn_slots_join(const WdSlots *s, void *stream);
int wdmpnn_slots_split(const WdSlots *s, void *stream);

/* Atom descriptors from a device-resident table (--atom_descriptors descriptor; mpn.py:77-79, 136-143).
 * `table` [table_rows][ld_table] holds the (already scaled) descriptor rows of a data split, d columns, the atoms
 * of a molecule on consecutive rows; row0[b] (int64, like wdmpnn_join_rows' indices) is the first table row of
 * batch molecule b.  atom_descriptors_layer is a Linear without an activation and the readout (mpn.py:145-171) is
 * linear in the atom rows, so with encoder dropout inactive the layer may run after the readout, on B rows instead
 * of n_atoms (c_a = Xn_b w_a / den_b; den_b = sum_a w_a for mean, 1 for sum, aggregation_norm for norm):
 *     readout([h | desc] W_d^T + b_d) = [readout(h) | readout(desc)] W_d^T + s_b b_d,     s_b = sum_a c_a
 * All four kernels: fp32 FMA, fixed thread-to-element maps, fixed summation orders (increasing index), no atomics,
 * plain vector stores: bitwise repeatable.  None of them clamps an index: row0[b] + mol_size[b] <= table_rows is
 * the caller's check (chemprop_amd.atom_descriptors validates every row on the host before it uploads row0).
 *
 * Join: one launch builds the layer's input x [B][ld_x], ld_x >= H + d + 1, from the descriptor-free encoder's
 * output emb [B][ld_emb] (H columns) and the graph g's mol_start, mol_size, w_atoms and degree_of_polym (B =
 * g->n_mols).  Per molecule b, atoms a = 0 .. mol_size[b] - 1 with weight w_a = w_atoms[mol_start[b] + a]:
 *     x[b][0 .. H)  = emb[b][0 .. H)                                            a pure copy (every bit)
 *     x[b][H + j]   = Xn_b * ((sum_a w_a table[row0[b] + a][j]) / den_b)        j < d, atoms in index order
 *     x[b][H + d]   = Xn_b * ((sum_a w_a) / den_b)                              s_b
 * The sum is formed first and divided afterwards, so a zero weight sum under mean gives the reference's NaN (a
 * molecule without atoms too: the Python side refuses those).  Columns of x at and beyond H + d + 1 are not written.
 * Refused before any launch: a NULL struct or graph, or emb, table, row0, x or one of the graph's four arrays NULL
 * with B > 0 (WD_ERR_ARG); B < 0, H <= 0, d <= 0, table_rows < 0, ld_emb < H, ld_table < d, ld_x < H + d + 1, an
 * unknown aggregation (WD_ERR_SHAPE); H + d > 4096 (WD_ERR_UNSUPPORTED).  B == 0 is a no-op. */
#define WD_DESC_MAX_WIDTH 4096
typedef struct WdDescJoin {
    const struct WdGraph *g;              /* n_mols, mol_start, mol_size, w_atoms, degree_of_polym */
    int32_t H, d;
    const float *emb; int32_t ld_emb;     /* [B][ld_emb]                                  */
    const float *table; int32_t ld_table; /* [table_rows][ld_table]                       */
    int64_t table_rows;
    const int64_t *row0;                  /* [B]                                          */
    int32_t aggregation;                  /* WdAggregation                                */
    float aggregation_norm;
    float *x; int32_t ld_x;               /* [B][ld_x]                                    */
} WdDescJoin;
int wdmpnn_desc_join(const WdDescJoin *j, void *stream);

/* Layer: y[b][i] = sum_{j < Hd} x[b][j] W_d[i][j] + x[b][Hd] b_d[i], i < Hd = H + d, in one launch of 16 x 16
 * tiles over (B, Hd).  W_d is nn.Linear.weight [Hd][Hd] row-major, b_d [Hd] or NULL (no bias term).  Columns of y at
 * and beyond Hd are not written.
 * Refused before any launch: a NULL struct, or x, W_d or y NULL with B > 0 (WD_ERR_ARG); B < 0, Hd <= 0,
 * ld_x < Hd + 1, ld_y < Hd (WD_ERR_SHAPE); Hd > WD_DESC_MAX_WIDTH, the heads' width limit (WD_ERR_UNSUPPORTED: the
 * caller keeps the per-atom layer).  B == 0 is a no-op. */
typedef struct WdDescLayer {
    int32_t B, Hd;
    const float *x; int32_t ld_x;         /* [B][ld_x]: Hd columns, then s                */
    const float *W_d, *b_d;
    float *y; int32_t ld_y;               /* [B][ld_y]                                    */
} WdDescLayer;
int wdmpnn_desc_layer(const WdDescLayer *l, void *stream);

/* Its backward from dy [B][ld_dy] and the same x, every output in ONE launch (the head stack's "dz | dW | db"):
 *     dW_d[i][j] = sum_b dy[b][i] x[b][j]              [Hd][Hd]
 *     db_d[i]    = sum_b dy[b][i] x[b][Hd]             [Hd]
 *     demb[b][h] = sum_i dy[b][i] W_d[i][h],  h < H    [B][ld_demb]: the encoder backward's input
 * Each of the three may be NULL ("not wanted": its tiles take no workgroups; all NULL launches nothing); every
 * wanted output is fully overwritten (no zeroing needed; with B == 0 nothing is written) and bitwise the same
 * whatever else is wanted.  Columns of demb at and beyond H are not written.
 * Refused before any launch: a NULL struct, or dy or x NULL with B > 0, or W_d NULL with B > 0 and demb wanted
 * (WD_ERR_ARG); B < 0, H <= 0, Hd < H, ld_dy < Hd, ld_x < Hd + 1, ld_demb < H with demb (WD_ERR_SHAPE);
 * Hd > WD_DESC_MAX_WIDTH (WD_ERR_UNSUPPORTED).  B == 0 is a no-op. */
typedef struct WdDescLayerBackward {
    int32_t B, H, Hd;
    const float *dy; int32_t ld_dy;
    const float *x; int32_t ld_x;
    const float *W_d;
    float *dW_d, *db_d;
    float *demb; int32_t ld_demb;
} WdDescLayerBackward;
int wdmpnn_desc_layer_backward(const WdDescLayerBackward *l, void *stream);

/* Rows: the padded per-atom array the per-atom descriptor path reads (WdGraph.atom_desc), for a training forward
 * with active encoder dropout, where nothing commutes: atom_desc [rows][ld], rows >= n_atoms rounded up to 128 and
 * ld >= d rounded up to 32 (the layout rule at the top of this header), from the same table in one launch:
 *     atom_desc[mol_start[b] + a][j] = table[row0[b] + a][j]        a < mol_size[b], j < d: a pure copy
 * and 0 everywhere else: row 0, rows outside every molecule, the rows at and beyond g->n_atoms, the columns at and
 * beyond d.  EVERY element of the buffer is written.  mol_start must be non-decreasing, as a_scope is.
 * Refused before any launch: a NULL struct or graph, or table, row0, atom_desc, mol_start or mol_size NULL with
 * B > 0 (WD_ERR_ARG); B < 0, d <= 0, table_rows < 0, ld_table < d, rows < n_atoms rounded up to 128, ld < d
 * rounded up to 32 (WD_ERR_SHAPE).  B == 0 is a no-op. */
typedef struct WdDescRows {
    const struct WdGraph *g;              /* n_mols, n_atoms, mol_start, mol_size          */
    int32_t d;
    const float *table; int32_t ld_table;
    int64_t table_rows;
    const int64_t *row0;                  /* [B]                                          */
    float *atom_desc; int32_t rows, ld;
} WdDescRows;
int wdmpnn_desc_rows(const WdDescRows *r, void *stream);

/* Ensembles (make_predictions.py:129-201): the per-cell mean and variance of the predictions of M models, and the
 * pairwise SID of an ensemble of spectra, accumulated on the device in double precision, which is what the
 * reference's numpy float64 sums of fp32 predictions are.  Both kernels are bandwidth-bound; no atomics, fixed
 * thread-to-element maps and reduction orders, plain vector stores.
 *
 * Add: folds model k's predictions of the data set's rows row0 .. row0 + B into the accumulators, one launch.
 * Per cell (b, c), c < W:
 *     v = (double)pred[b][c] * scale_std[c] + scale_mean[c]     (a rounded product, then a rounded sum: bitwise
 *                                                                 scaler.py's inverse_transform in numpy; without
 *                                                                 the two scale pointers v = (double)pred[b][c])
 *     k == 0:  mean = v, m2 = 0                                  (the buffers need no zeroing)
 *     k  > 0:  d = v - mean;  mean += d / (k + 1);  m2 += d * (v - mean)         (Welford)
 * on mean[row0 + b][c] and m2[row0 + b][c]; keep[row0 + b][c] = v when `keep` (this model's slab) is given.
 * m2 / M is the population variance (np.var).  A NaN v makes its own cell NaN and no other.  Columns at and beyond
 * W of the accumulators are not written.
 * Refused before any launch: a NULL struct, or pred or mean NULL with B > 0 (WD_ERR_ARG); B < 0, W <= 0,
 * ld_pred < W, ld_acc < W, row0 < 0, k < 0, exactly one of the scale pointers (WD_ERR_SHAPE);
 * k >= WD_ENSEMBLE_MAX_MODELS (WD_ERR_UNSUPPORTED).  B == 0 is a no-op. */
#define WD_ENSEMBLE_MAX_MODELS 32
typedef struct WdEnsembleAdd {
    const float *pred;        /* [B][ld_pred], W columns used                       */
    int32_t ld_pred, B, W;
    int32_t k;                /* 0-based index of this model                        */
    int64_t row0;             /* first row of the accumulators this block covers    */
    const double *scale_mean; /* [W] the model's target scaler, or both NULL        */
    const double *scale_std;
    double *mean;             /* [rows][ld_acc]                                     */
    double *m2;               /* [rows][ld_acc], or NULL                            */
    double *keep;             /* this model's slab [rows][ld_acc], or NULL          */
    int32_t ld_acc;
} WdEnsembleAdd;
int wdmpnn_ensemble_add(const WdEnsembleAdd *e, void *stream);

/* Pairwise SID: roundrobin_sid (spectra_utils.py:211-241) of the kept slabs, value of model m, row n, position t
 * at preds[m * model_stride + n * ld + t].  Its head / tail concatenation holds every unordered pair once:
 *     out[n] = 1 / (M (M - 1) / 2) * sum over a < b, over t, of (p_a - p_b) (log p_a - log p_b)
 * Positions where model 0 holds NaN contribute 0 (the reference's nan_mask); with threshold > 0 every value below
 * it is raised to it first (threshold <= 0: off); M == 1 gives NaN, the reference's mean over no pairs.  One
 * workgroup per row; each position's M logs are computed once.  Elements of `out` at and beyond N are not written.
 * Refused before any launch: a NULL struct (WD_ERR_ARG); M < 1, T < 1, N < 0, ld < T, model_stride < N * ld
 * (WD_ERR_SHAPE); M > WD_ENSEMBLE_MAX_MODELS (WD_ERR_UNSUPPORTED); preds or out NULL with N > 0 (WD_ERR_ARG).
 * N == 0 is a no-op. */
typedef struct WdEnsembleSid {
    const double *preds;
    int64_t model_stride;     /* elements between two models' slabs                 */
    int32_t ld, M, N, T;
    double threshold;
    double *out;              /* [N]                                                */
} WdEnsembleSid;
int wdmpnn_ensemble_sid(const WdEnsembleSid *e, void *stream);

/* Latent vectors of an ensemble (molecule_fingerprint.py:90-117, make_predictions.py:156-195): folds model k's fp32
 * rows into the accumulators in one launch.  Per cell (b, c), c < W, with v = src[b * ld_src + c0 + c]:
 *     cols[((row0 + b) * W + c) * M + k] = (double)v      when cols is given: the reference's
 *                                                          all_fingerprints[N][W][M]
 *     sum[(row0 + b) * ld_sum + c]  = v                    when sum is given and k == 0 (no zeroing needed)
 *     sum[(row0 + b) * ld_sum + c] += v                    when sum is given and k > 0: one fp32 add, so the sum over
 *                                                          the models in order is bitwise numpy's fp32 running sum
 * c0 skips leading columns of src, W drops trailing ones (the feature columns behind an encoding) without a copy.
 * One thread per cell, a fixed thread-to-element map, no atomics, plain vector stores; a NaN stays in its own cell;
 * columns of sum at and beyond W are not written.
 * Refused before any launch: a NULL struct, src NULL with B > 0, cols and sum both NULL (WD_ERR_ARG); B < 0, W <= 0,
 * c0 < 0, ld_src < c0 + W, ld_sum < W with a sum, row0 < 0, M < 1, k outside [0, M) (WD_ERR_SHAPE);
 * M > WD_ENSEMBLE_MAX_MODELS (WD_ERR_UNSUPPORTED).  B == 0 is a no-op. */
typedef struct WdLatentAdd {
    const float *src;         /* [B][ld_src], columns c0 .. c0 + W used             */
    int32_t ld_src, B, W, c0;
    int32_t M, k;             /* models in all, 0-based index of this one           */
    int64_t row0;             /* first row of the accumulators this block covers    */
    double *cols;             /* [rows][W][M], or NULL                              */
    float *sum;               /* [rows][ld_sum], or NULL                            */
    int32_t ld_sum;
} WdLatentAdd;
int wdmpnn_latent_add(const WdLatentAdd *e, void *stream);

/* Scoring a split on the device (evaluate.py:11-77 over predict.py:10-68): the sums behind rmse, mse, mae, r2,
 * cross_entropy and accuracy, the per-row SID / Wasserstein terms of spectra, and ROC AUC by counting, from the fp32
 * predictions of the native prediction heads against a target table that stays on the device: double
 * targets[N][ld_targets], NaN = missing, a multiclass entry = the class index.  Double precision throughout, every
 * operation rounded on its own where the host code it replaces rounds; no atomics, fixed thread-to-element maps and
 * reduction orders, plain vector stores.
 *
 * Add: folds the batch pred[B][tasks * classes] (rows row0 .. row0 + B of the split) into partials[tasks][WD_EVAL_SLOTS],
 * which the caller zeroes once; one workgroup per task, a batch's terms reduced over a fixed tree and then added to
 * the running partials, so launches on one stream are sequenced.  With `keep`, also stores the value v of every cell
 * (present target or not) at keep[row0 + b][c], as float (keep_f32 != 0) or double.  Per present target t:
 *   WD_EVAL_REGRESSION      v = (double)pred * scale_std[task] + scale_mean[task] (a rounded product, then a rounded
 *                           sum; v = (double)pred without the scale pointers); e = v - t;
 *                           slot 0 += e e, slot 1 += |e|
 *   WD_EVAL_CLASSIFICATION  p = (double)pred, eps = 2^-52;
 *                           slot 0 += -log(clip(p, eps, 1 - eps)) for t == 1, -log(clip(1 - p, eps, 1 - eps)) otherwise
 *                           (sklearn's log_loss); slot 1 += [(p > 0.5) == (t == 1)]; slot 2 += [p == 0];
 *                           slot 3 += [p == 1]
 *   WD_EVAL_MULTICLASS      the task's `classes` probabilities p[.]: slot 0 += -log(clip(p[t], eps, 1 - eps));
 *                           slot 1 += [first maximum of p[.] == t].  A present t must be an integer in
 *                           [0, classes): the caller checks the table when it builds it.
 * Refused before any launch: a NULL struct (WD_ERR_ARG); an unknown kind, B < 0, tasks < 1, classes < 1, classes != 1
 * unless multiclass, ld_pred < tasks * classes, ld_targets < tasks, a keep with ld_keep < tasks * classes, row0 < 0,
 * row0 + B > N, exactly one of the scale pointers, scale pointers for another kind than regression (WD_ERR_SHAPE);
 * pred, targets or partials NULL with B > 0 (WD_ERR_ARG).  B == 0 is a no-op. */
#define WD_EVAL_SLOTS 4
#define WD_EVAL_REGRESSION 0
#define WD_EVAL_CLASSIFICATION 1
#define WD_EVAL_MULTICLASS 2
typedef struct WdEvalAdd {
    const float *pred;        /* [B][ld_pred], tasks * classes columns used          */
    int32_t ld_pred, B, tasks, classes;
    int32_t kind;             /* WD_EVAL_*                                           */
    int32_t ld_targets;
    int64_t row0, N;          /* the batch's first row; the rows of the split        */
    const double *targets;    /* [N][ld_targets]                                     */
    const double *scale_mean; /* [tasks] the target scaler (regression), or both NULL */
    const double *scale_std;
    double *partials;         /* [tasks][WD_EVAL_SLOTS]                              */
    void *keep;               /* [N][ld_keep] float or double, or NULL               */
    int32_t ld_keep, keep_f32;
} WdEvalAdd;
int wdmpnn_eval_add(const WdEvalAdd *e, void *stream);

/* Spectra: one workgroup per row of the batch writes sid[row0 + b] and / or wasserstein[row0 + b] (either may be
 * NULL), spectra_utils.py:42-83 / 117-159 per row.  pred arrives normalised, NaN where the row's phase excludes the
 * position; a position counts where its target is present.  z = pred where present and not NaN, else 0; p = z / sum z;
 *     sid         = sum over the present positions of p log(p / y) + y log(y / p)
 *     wasserstein = sum over all positions t of |cumsum(y)_t - cumsum(p)_t|, a missing y as 0
 * Each of the 256 threads takes a contiguous chunk of ceil(T / 256) positions; the chunk sums of p and y are scanned
 * over LDS in index order, and a second pass forms the terms.  With `keep`, stores pred as it came.
 * Refused before any launch: a NULL struct (WD_ERR_ARG); B < 0, T < 1, ld_pred < T, ld_targets < T, a keep with
 * ld_keep < T, row0 < 0, row0 + B > N (WD_ERR_SHAPE); T > WD_HEAD_MAX_SPECTRUM (WD_ERR_UNSUPPORTED); pred or targets
 * NULL, or both outputs NULL, with B > 0 (WD_ERR_ARG).  B == 0 is a no-op. */
typedef struct WdEvalSpectra {
    const float *pred;        /* [B][ld_pred]                                        */
    int32_t ld_pred, B, T, ld_targets;
    int64_t row0, N;
    const double *targets;    /* [N][ld_targets]                                     */
    double *sid;              /* [N], or NULL                                        */
    double *wasserstein;      /* [N], or NULL                                        */
    void *keep;               /* [N][ld_keep] float or double, or NULL               */
    int32_t ld_keep, keep_f32;
} WdEvalSpectra;
int wdmpnn_eval_spectra(const WdEvalSpectra *e, void *stream);

/* ROC AUC by counting, from the kept predictions preds[N][ld_preds] (float when preds_f32, else double; column =
 * task) and the target table.  Grid (task, block of 256 rows): a thread holds one row i with t_i == 1 and streams
 * every row j through LDS in tiles of 256, counting 2 [t_j == 0 and p_j < p_i] + [t_j == 0 and p_j == p_i]; a block
 * reduction writes counts[task][block], blocks = ceil(N / 256).  The caller sums a task's integers and divides by
 * 2 P Nneg (P rows with t == 1, Nneg with t == 0): a tie counts one half, as the trapezoid rule gives it, and
 * integer sums do not depend on any order.
 * Refused before any launch: a NULL struct (WD_ERR_ARG); N < 0, tasks < 1, ld_preds < tasks, ld_targets < tasks
 * (WD_ERR_SHAPE); N > WD_EVAL_AUC_MAX_ROWS (WD_ERR_UNSUPPORTED: a count must fit 64 bits, and the work is
 * quadratic) or tasks > 65535 (the grid's second dimension); preds, targets or counts NULL with N > 0 (WD_ERR_ARG).  N == 0 is a no-op. */
#define WD_EVAL_AUC_MAX_ROWS (1 << 24)
typedef struct WdEvalAuc {
    const void *preds;        /* [N][ld_preds]                                       */
    const double *targets;    /* [N][ld_targets]                                     */
    int64_t N;
    int32_t tasks, ld_preds, ld_targets, preds_f32;
    int64_t *counts;          /* [tasks][ceil(N / 256)]                              */
} WdEvalAuc;
int wdmpnn_eval_auc(const WdEvalAuc *e, void *stream);

/* One Adam / AdamW optimizer step (torch.optim.Adam / AdamW semantics without amsgrad: the optimizer
 * step of train/train.py:84, built by utils.py:295-310) over n tensors in one launch per 16 tensors.
 * Replaces torch's multi-tensor / fused Adam kernels; per element: g += wd p (AdamW: p -= lr wd p),
 * m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2, p -= lr / (1 - b1^step) * m / (sqrt(v) /
 * sqrt(1 - b2^step) + eps).  step is the 1-based step count after this update.  Every pointer is a
 * device pointer to contiguous fp32 data; tensors with numel 0 are skipped. */
typedef struct WdAdamTensor {
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    int64_t numel;
} WdAdamTensor;
typedef struct WdAdamHyper {
    float lr, beta1, beta2, eps, weight_decay;
    int32_t step;         /* >= 1 */
    int32_t decoupled;    /* 1 = AdamW */
} WdAdamHyper;
int wdmpnn_adam_step(const WdAdamTensor *tensors, int32_t n, const WdAdamHyper *h, void *stream);
/* The same step, also rewriting the encoder's packed weights (wdmpnn_pack_params layout for g, p, c) from
 * the updated values: the copies the next training forward and backward read (padded plain, transposed,
 * bf16x3 plane tiles, W_h's fp16-pair tiles and scale) come out of the optimizer's own pass instead of a
 * pack before every forward (train.py:84 then mpn.py:66's next call).  tensors must hold p's W_i, b_i,
 * W_h, b_h, W_o and b_o (matched by param pointer, with their full sizes) and `packed` must hold a pack of
 * their previous values (its zero padding is kept); bond messages without descriptors only
 * (WD_ERR_UNSUPPORTED otherwise: pack after the plain step).  Afterwards `packed` equals a fresh
 * wdmpnn_pack_params of the updated weights bytewise except W_h's partial scale words (the per-workgroup
 * maxima before word 64, and the per-tile words after it, are the optimizer's, not pack_kernel's); the
 * folded word 64, the one every consumer reads, is equal. */
int wdmpnn_adam_step_repack(const WdAdamTensor *tensors, int32_t n, const WdAdamHyper *h, const WdGraph *g,
                            const WdParams *p, const WdConfig *c, void *packed, size_t packed_bytes, void *stream);

/* The training step's FFN head + masked loss and their gradients in two launches (model.py:57-121
 * with ffn_num_layers = 2 and no dropout, train.py:55-74 with MSELoss, BCEWithLogitsLoss or per-task
 * CrossEntropyLoss): replaces the ~25 small torch ops (and their host time) of ffn(emb),
 * loss_func(preds, targets) * weights, .sum() / mask.sum() and their autograd backward.  Row-major fp32
 * device arrays; w = target weight * data weight * mask per entry.
 * Multiclass (loss_kind 2, ABI 12): the T outputs are tasks = T / n_classes groups of n_classes logits
 * (model.py:189-190's reshape), the table holds one target per TASK -- the class index as a float -- and
 * one weight per task: [B][ld_table] with ld_table >= 2 * tasks.  Per task, with m = max_c s_c and
 * lse = m + log(sum_c exp(s_c - m)): loss += w (lse - s_y), dout[c] = w (exp(s_c - lse) - [c == y]) / n
 * (the max-subtracted form: finite for any finite logits).  The class index is only compared, never used
 * as an address: an index outside [0, n_classes) gives a wrong number, not a fault.  Requires
 * n_classes >= 2 and T % n_classes == 0 (WD_ERR_SHAPE otherwise); kinds 0 and 1 require n_classes == 1.
 * T <= 64 outputs in every kind (WD_ERR_UNSUPPORTED beyond). */
typedef struct WdHead {
    const float *x; int32_t ld_x;          /* encoder output [B][ld_x], first F columns used        */
    int32_t B, F, Hf, T;                   /* rows, input width, hidden width, FFN outputs (rows of W2) */
    const float *W1, *b1, *W2, *b2;        /* nn.Linear(F, Hf), nn.Linear(Hf, T) (biases may be NULL) */
    const float *table; int32_t ld_table;  /* [B][ld_table]: targets [T / n_classes], then weights w */
    float inv_n;                           /* 1 / mask.sum()                                        */
    int32_t act;                           /* WdActivation of the FFN (not PReLU)                   */
    float *a, *dh, *dout, *lossrow;        /* scratch [B][Hf], [B][Hf], [B][T], [B]                 */
    float *dx;                             /* [B][ld_x]: d loss / d x                               */
    float *dW1, *db1, *dW2, *db2;          /* parameter gradients (db1 / db2 NULL = skip)           */
    float *loss;                           /* [1]                                                   */
    int32_t loss_kind;                     /* 0: MSELoss (regression), 1: BCEWithLogitsLoss         */
                                           /* (classification: the FFN's logits, train.py:55-74 with */
                                           /* utils.py get_loss_func; sigmoid only at eval),          */
                                           /* 2: CrossEntropyLoss per task (multiclass)               */
    int32_t n_classes;                     /* classes per task: 1 for kinds 0 and 1, >= 2 for kind 2 */
} WdHead;
int wdmpnn_head_mse(const WdHead *h, void *stream);
/* The same FFN at prediction time (model.py:152-194 in eval mode): the kernels of wdmpnn_head_stack_predict
 * at L = 2 (a is their z_1), still two launches and the same bits: out = W2 act(W1 x +
 * b1) + b2 followed by out_kind 0: nothing (regression), 1: sigmoid (classification, model.py:186-188),
 * 2: softmax over each group of n_classes consecutive outputs (multiclass, model.py:189-192;
 * max-subtracted).  Same size limits, activations and argument checks as wdmpnn_head_mse (n_classes == 1
 * for kinds 0 and 1; n_classes >= 2 dividing T for kind 2).  B == 0 is a no-op. */
typedef struct WdHeadPredict {
    const float *x; int32_t ld_x;          /* encoder output [B][ld_x], first F columns used        */
    int32_t B, F, Hf, T;                   /* rows, input width, hidden width, FFN outputs          */
    const float *W1, *b1, *W2, *b2;        /* nn.Linear(F, Hf), nn.Linear(Hf, T) (biases may be NULL) */
    int32_t act;                           /* WdActivation of the FFN (not PReLU)                   */
    float *a;                              /* scratch [B][Hf]                                       */
    float *out;                            /* [B][T]                                                */
    int32_t out_kind;                      /* 0 identity, 1 sigmoid, 2 softmax per class group      */
    int32_t n_classes;                     /* 1 for kinds 0 and 1, >= 2 for kind 2                  */
} WdHeadPredict;
int wdmpnn_head_predict(const WdHeadPredict *h, void *stream);
/* p_i[0 .. n_i) *= *s (device scalar) for k <= 8 buffers: the head's gradients times the loss's
 * incoming gradient in one launch. */
int wdmpnn_scale(float *const *p, const int64_t *n, int32_t k, const float *s, void *stream);

/* The FFN head in full generality (model.py:57-121 with any ffn_num_layers, active dropout, any of the six
 * activations): L nn.Linear layers of widths F -> Hf -> ... -> Hf -> T (L == 1: F -> T),
 *     a_0 = drop_0(x),  z_l = a_{l-1} W_l^T + b_l (l = 1 .. L),  a_l = drop_l(act(z_l)) (l = 1 .. L-1),
 *     out = z_L,
 * the losses of WdHead (loss_kind, n_classes, table, ld_table, inv_n: exactly as there) and every gradient in
 * one call: dx, dW_l, db_l and, for PReLU, dslope (ONE slope shared by every activation site, as the
 * reference's single activation module: its gradient is the sum over the sites).
 * Dropout: drop_l(v)[row][col] = v[row][col] * m, m = 0 or 1 / (1 - p), the counter hash of
 * (seed, layer = l, row, col) -- chemprop_amd.nn_utils.dropout_mask restates it.  Site l has the shape of
 * Linear l+1's input; no mask is stored (the backward re-derives it); p == 0 skips the hash.
 * 2 L - 1 launches (2 for L == 1): one GEMM per hidden layer with the activation and the mask applied as its
 * A operand is staged, one row kernel (the last layer, the loss, dz_{L-1}), then one launch per layer
 * L-1 .. 1 for dz_{l-1} | dW_l | db_l (the last layer's dW_L, db_L and the loss ride in the first of them).
 * Fixed summation orders and no float atomics: bitwise repeatable.  fp32 FMA.
 * Limits: 1 <= L <= WD_HEAD_MAX_LAYERS, F and Hf <= 4096, T <= 64 (WD_ERR_UNSUPPORTED beyond); 0 <= p < 1.
 * scratch: caller-owned device memory of at least wdmpnn_head_stack_scratch_bytes (16-byte aligned).
 * B == 0 is a no-op. */
#define WD_HEAD_MAX_LAYERS 6
typedef struct WdHeadStack {
    const float *x; int32_t ld_x;          /* encoder output [B][ld_x], first F columns used        */
    int32_t B, F, Hf, T, L;                /* rows, input width, hidden width, outputs, Linear layers */
    const float *W[WD_HEAD_MAX_LAYERS];    /* W_l: [out_l][in_l] row-major (nn.Linear.weight)       */
    const float *b[WD_HEAD_MAX_LAYERS];    /* b_l or NULL                                           */
    const float *slope;                    /* [1]: PReLU's slope (act == WD_ACT_PRELU), else unused */
    const float *table; int32_t ld_table;  /* as WdHead (may be pinned host memory)                 */
    float inv_n;                           /* 1 / mask.sum()                                        */
    int32_t act;                           /* WdActivation (any of the six)                         */
    float p;                               /* dropout probability of every site (0: none)           */
    uint64_t seed;                         /* the head's dropout seed                               */
    int32_t loss_kind, n_classes;          /* as WdHead                                             */
    void *scratch; size_t scratch_bytes;
    float *out;                            /* [B][T]: the FFN's outputs z_L, or NULL                */
    float *dx;                             /* [B][ld_x]: d loss / d x                               */
    float *dW[WD_HEAD_MAX_LAYERS];         /* d loss / d W_l                                        */
    float *db[WD_HEAD_MAX_LAYERS];         /* d loss / d b_l (NULL = skip)                          */
    float *dslope;                         /* [1] (NULL = skip; 0 is written unless PReLU and L > 1) */
    float *loss;                           /* [1]                                                   */
} WdHeadStack;
/* floats: z_l and dz_l [B][Hf] for l = 1 .. L-1, a_{L-1} [B][L == 1 ? F : Hf], dout [B][T], the rows'
 * loss terms [B], and (L - 1) x max(B, ceil(B / 16) ceil(Hf / 16)) partial sums of dslope. */
int wdmpnn_head_stack_scratch_bytes(int32_t B, int32_t F, int32_t Hf, int32_t T, int32_t L, size_t *bytes);
int wdmpnn_head_stack(const WdHeadStack *h, void *stream);
/* The same head for a partly frozen model: any subset of the gradients.  Same struct, forward, losses, dropout
 * hash and scratch as wdmpnn_head_stack; dx, every dW[l], every db[l] and dslope may each be NULL ("not
 * wanted"), independently.  loss is always written.  Every wanted output is bitwise what wdmpnn_head_stack
 * writes for it (fixed summation orders: no output depends on which others are computed).  What nobody wants
 * is not launched: the dz chain runs down to level 0 only for dx, to level 1 for PReLU's dslope, else to the
 * first layer with a wanted dW or db; a layer's dW tiles, its db sums and the dz tiles below that level take no
 * workgroups; a launch left with nothing is dropped, and when no launch of a layer below L remains, dW_L, db_L
 * and the loss get a small launch of their own.  Nothing is read or written through a NULL pointer; the scratch
 * regions of skipped levels stay unused.  Refusals: those of wdmpnn_head_stack but for its null-gradient ones
 * (W, loss, scratch, and with B > 0 x and table, are still required).  B == 0 is a no-op. */
int wdmpnn_head_stack_partial(const WdHeadStack *h, void *stream);
/* The same stack at prediction time (eval mode: no dropout) in L launches, with the output kinds of
 * WdHeadPredict.  scratch: (L - 1) B Hf floats (the z_l), at least scratch_bytes of them given. */
typedef struct WdHeadStackPredict {
    const float *x; int32_t ld_x;
    int32_t B, F, Hf, T, L;
    const float *W[WD_HEAD_MAX_LAYERS];
    const float *b[WD_HEAD_MAX_LAYERS];
    const float *slope;
    int32_t act;
    void *scratch; size_t scratch_bytes;
    float *out;                            /* [B][T]                                                */
    int32_t out_kind;                      /* 0 identity, 1 sigmoid, 2 softmax per class group      */
    int32_t n_classes;                     /* 1 for kinds 0 and 1, >= 2 for kind 2                  */
} WdHeadStackPredict;
int wdmpnn_head_stack_predict(const WdHeadStackPredict *h, void *stream);
/* The latent vector of the same stack (model.py:123-150, fingerprint_type 'last_FFN'): the input of the FFN's last
 * Linear in eval mode,
 *     z_1 = x W_1^T + b_1,  z_l = act(z_{l-1}) W_l^T + b_l (l = 2 .. L-1),  out = act(z_{L-1}),
 * as [B][ld_out], first Hf columns.  L - 1 launches: the first L - 2 are the launches wdmpnn_head_stack_predict
 * makes (the same tile code: their z_l in the scratch are bitwise the same), the last one is layer L-1's with the
 * activation applied as its tile is stored, straight into out.  No dropout, no output kind, no T; W[L-1] and
 * b[L-1] are not read.  scratch: (L - 2) B Hf floats (NULL allowed for L == 2).  Columns of out at and beyond Hf
 * are not written.  Refused before any launch: a NULL struct (WD_ERR_ARG); L < 2: there is no latent layer
 * (WD_ERR_SHAPE); L > WD_HEAD_MAX_LAYERS, F or Hf > 4096, an unknown activation (WD_ERR_UNSUPPORTED); B < 0,
 * F <= 0, Hf <= 0, ld_x < F, ld_out < Hf (WD_ERR_SHAPE); PReLU without its slope, or x, out or one of W_1 ..
 * W_{L-1} NULL with B > 0 (WD_ERR_ARG); a scratch too small (WD_ERR_WORKSPACE).  B == 0 is a no-op. */
typedef struct WdHeadLatent {
    const float *x; int32_t ld_x;
    int32_t B, F, Hf, L;
    const float *W[WD_HEAD_MAX_LAYERS];
    const float *b[WD_HEAD_MAX_LAYERS];
    const float *slope;
    int32_t act;
    void *scratch; size_t scratch_bytes;
    float *out; int32_t ld_out;            /* [B][ld_out], Hf columns written                       */
} WdHeadLatent;
int wdmpnn_head_stack_latent(const WdHeadLatent *h, void *stream);

/* The spectra head (dataset_type spectra, model.py:102-113, train.py:70-74, spectra_utils.py): the FFN of
 * WdHeadStack (same x, layers, activation, slope, dropout hash, seed, scratch contract and gradient outputs)
 * with up to WD_HEAD_MAX_SPECTRUM outputs, one per spectrum bin, the output activation s = act_s(z_L)
 * (spectra_act 0: exp, 1: softplus) and a row loss on the masked, row-normalised output:
 *     m_t = [target_t present],  S = sum_t m_t s_t,  p_t = m_t s_t / S,
 *     loss_kind 0 (SID):          sum_t w_t (p_t - y_t) (log p_t - log y_t)
 *     loss_kind 1 (Wasserstein):  sum_t w_t |cumsum(y)_t - cumsum(p)_t|
 * summed over the rows and times inv_n.  table: [B][ld_table], targets [T] then weights w [T] (target weight *
 * data weight * mask) as WdHead, device memory (each row is read in several passes); a target of exactly 0
 * means "missing" (every present target is > 0 after normalize_spectra's floor): the mask comes from the
 * targets, never from w, so a present target with weight 0 still counts in S.  exp: p and log p are the
 * max-subtracted softmax over the present positions (finite for any finite logits); softplus:
 * max(z, 0) + log1p(exp(-|z|)).  A row without a present target contributes loss 0 and gradient 0 (the
 * reference: NaN).  out (or NULL) receives act_s(z_L), what the model returns in training mode.
 * dx, every dW[l], every db[l] and dslope may each be NULL ("not wanted"), as wdmpnn_head_stack_partial; loss
 * is always written; every wanted output is bitwise the same whatever else is wanted.  Launches: one GEMM per
 * hidden layer, the last layer as 16 x 16 tiles over (B, T), one workgroup per row for the loss and
 * d loss / d z_L, one launch for dz_{L-1} | dW_L | db_L | loss, then one per layer L-1 .. 1.  Fixed summation
 * and scan orders, no float atomics.  Limits: 1 <= L <= WD_HEAD_MAX_LAYERS, F and Hf <= 4096,
 * 1 <= T <= WD_HEAD_MAX_SPECTRUM (WD_ERR_UNSUPPORTED beyond), ld_table >= 2 T, 0 <= p < 1.  B == 0 is a no-op. */
#define WD_HEAD_MAX_SPECTRUM 8192
typedef struct WdHeadSpectra {
    const float *x; int32_t ld_x;
    int32_t B, F, Hf, T, L;
    const float *W[WD_HEAD_MAX_LAYERS];
    const float *b[WD_HEAD_MAX_LAYERS];
    const float *slope;
    const float *table; int32_t ld_table;  /* [B][ld_table]: targets [T] (0 = missing), then weights w [T] */
    float inv_n;
    int32_t act;
    float p;
    uint64_t seed;
    int32_t spectra_act;                   /* 0 exp, 1 softplus                                     */
    int32_t loss_kind;                     /* 0 SID, 1 Wasserstein                                  */
    void *scratch; size_t scratch_bytes;
    float *out;                            /* [B][T]: act_s(z_L), or NULL                           */
    float *dx;                             /* [B][ld_x] or NULL                                     */
    float *dW[WD_HEAD_MAX_LAYERS];         /* NULL = not wanted                                     */
    float *db[WD_HEAD_MAX_LAYERS];
    float *dslope;
    float *loss;                           /* [1]                                                   */
} WdHeadSpectra;
/* floats: those of wdmpnn_head_stack_scratch_bytes, then z_L - b_L [B][T] (the row kernels add the bias: the
 * softmax's differences are taken product and bias apart, so a large bias costs no precision). */
int wdmpnn_head_spectra_scratch_bytes(int32_t B, int32_t F, int32_t Hf, int32_t T, int32_t L, size_t *bytes);
int wdmpnn_head_spectra(const WdHeadSpectra *h, void *stream);
/* The same head at prediction time (eval mode: no dropout), L + 1 launches.  normalize 0: out = act_s(z_L);
 * 1: each row divided by the sum of its included positions (spectra_utils.normalize_spectra; mask [B][T],
 * nonzero = included, NULL = all), excluded positions written as quiet NaN.
 * scratch: (L - 1) B Hf + B T floats (the z_l, then z_L - b_L). */
typedef struct WdHeadSpectraPredict {
    const float *x; int32_t ld_x;
    int32_t B, F, Hf, T, L;
    const float *W[WD_HEAD_MAX_LAYERS];
    const float *b[WD_HEAD_MAX_LAYERS];
    const float *slope;
    int32_t act;
    void *scratch; size_t scratch_bytes;
    float *out;                            /* [B][T]                                                */
    int32_t spectra_act;                   /* 0 exp, 1 softplus                                     */
    int32_t normalize;
    const uint8_t *mask;
} WdHeadSpectraPredict;
int wdmpnn_head_spectra_predict(const WdHeadSpectraPredict *h, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Native streamed batches (BASELINE.json configs[4]: millions of synthetic polymer graphs per rank,
 * never materialised).  Replaces chemprop's DataLoader + construct_molecule_batch + BatchMolGraph
 * (data.py:594-607, featurization.py:757-813) for the synthetic stream, and the per-batch
 * MPNEncoder.forward host work (mpn.py:77-90): generator threads stage compact batches into pinned
 * slots, a feed thread uploads them and builds each device graph (wdmpnn_build_graph_ex) on its own
 * stream, the caller's stream only waits on each graph's ready event.  Batch i is generated from
 * seed + i (mix the rank into the seed for disjoint shards) and handed out in order.
 * ------------------------------------------------------------------------------------------------ */
typedef struct WdFeedSpec {
    int32_t kind;           /* synthetic generator: 0 polymer, 1 QM9-like, 2 ZINC-like */
    int32_t batch;          /* graphs per batch */
    int64_t n_batches;
    uint64_t seed;          /* batch i: seed + i */
    int32_t producers;      /* generator threads (>= 1) */
    int32_t slots;          /* batches in flight: host and device slots (>= 2) */
    int32_t target_blocks;  /* molecule-block plan target (>= 1) */
    int32_t flags;          /* WDMPNN_GRAPH_LEAN: inference-only device graphs; WDMPNN_GRAPH_NO_PLANES */
    int32_t atom_fdim, bond_fdim;
    void *pinned;           /* caller-owned pinned host memory: slots x host slot bytes */
    void *device;           /* caller-owned device memory: slots x device slot bytes, 256-byte aligned */
} WdFeedSpec;
typedef struct WdFeedBatch {
    int64_t index;
    int32_t n_mols, n_atoms, n_bonds, n_blocks, nnz_msg, reserved;
    size_t h2d_bytes;       /* the staged image uploaded for this batch */
} WdFeedBatch;
int wdmpnn_feed_slot_bytes(int32_t kind, int32_t batch, int32_t atom_fdim, int32_t bond_fdim, size_t *host_bytes,
                           size_t *device_bytes);
int wdmpnn_feed_create(const WdFeedSpec *spec, void **feed);
/* The next batch: blocks until its graph has been enqueued, makes `stream` wait for it on the GPU and
 * returns its WdGraph (device pointers into the feed's slot, valid until released).  Returns 1 when the
 * stream is exhausted, 0 on success, < 0 on error (a producer's error included). */
int wdmpnn_feed_next(void *feed, void *stream, WdGraph *g, WdFeedBatch *info);
/* Every batch handed out so far is finished when `stream` reaches this point: their slots are reused
 * after it (the feed's own thread waits for that point before refilling a slot; the caller's thread
 * does not block, and no stream waits on `stream`). */
int wdmpnn_feed_release(void *feed, void *stream);
/* Workspace of wdmpnn_feed_forward for up to k batches of this feed. */
int wdmpnn_feed_forward_workspace_bytes(void *feed, const WdParams *p, const WdConfig *c, int32_t k, size_t *bytes);
/* Up to k next batches through the fused inference forward in one launch set (wdmpnn_forward_many),
 * then released: outputs [sum n_mols, H] into out (out_rows available), *got batches (0 = exhausted),
 * *rows output rows, *edges directed real edges, *h2d_bytes bytes uploaded for them. */
int wdmpnn_feed_forward(void *feed, int32_t k, const WdParams *p, const WdConfig *c, void *workspace,
                        size_t workspace_bytes, float *out, int64_t out_rows, void *stream, int32_t *got,
                        int64_t *rows, int64_t *edges, int64_t *h2d_bytes);
int wdmpnn_feed_destroy(void *feed);

#ifdef __cplusplus
}
#endif
#endif /* WDMPNN_H */
